// Runs a file of preset dictionaries and stored LZ4 blocks through the
// host-compiled decoders of toplingdb_amd/csrc/dcw_lz4_dec.h with an Lz4Dict —
// the very source k_decompress_lz4_dict compiles — and compares with the
// record.  Build as a stand-alone program with
//   g++ -O1 -g -fsanitize=address,undefined -I toplingdb_amd/csrc
//       tools/lz4_dict_host/lz4_dict_host.cpp -o lz4_dict_host
//
//   lz4_dict_host <file>
// file: records as tools/lz4_host reads them (explen == 0xffffffff: every
// decoder must refuse); a record with usize == 0xfffffffe is a dictionary of n
// bytes for the records behind it.
//
// lz4_dec_lds runs on blocks within DEC_MAX on both sides in buffers of
// exactly DEC_MAX + DEC_PAD heap bytes, the slack behind the input once 0xff
// and once 0x00; lz4_dec on heap buffers of exactly n and usize bytes.  The
// dictionary is a heap object of its exact size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define __device__
#define __forceinline__ inline
#define DCW_LZ4_LDS_ON_HOST
#include "dcw_lz4_dec.h"

#define DEC_MAX 4992 // dcw_k_decode.h
#define DEC_PAD 16

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  uint32_t hdr[3];
  int rec = 0, bad = 0, refused = 0, lds_runs = 0, dicts = 0;
  uint8_t* dbuf = nullptr;
  dcw::Lz4Dict dict = {nullptr, 0};
  while (fread(hdr, 4, 3, f) == 3) {
    uint32_t n = hdr[0], usize = hdr[1], explen = hdr[2];
    if (usize == 0xfffffffeu) {
      free(dbuf);
      dbuf = (uint8_t*)malloc(n ? n : 1);
      if (fread(dbuf, 1, n, f) != n) return 2;
      dict.e = dbuf + n; // as k_decompress_lz4_dict sets it up
      dict.n = n < 65535u ? n : 65535u;
      dicts++;
      continue;
    }
    bool malformed = explen == 0xffffffffu;
    uint8_t* payload = (uint8_t*)malloc(n ? n : 1);
    uint8_t* want = (uint8_t*)malloc(malformed || !explen ? 1 : explen);
    if (fread(payload, 1, n, f) != n) return 2;
    if (!malformed && explen && fread(want, 1, explen, f) != explen) return 2;
    uint32_t us = 0;
    int hn = dcw::lz4_preamble(payload, n, &us);
    if (hn < 0 || us > (64u << 20)) {
      if (!malformed) { printf("rec %d: preamble refused\n", rec); bad++; }
    } else {
      if (!malformed && us != usize) { printf("rec %d: usize %u\n", rec, us); bad++; }
      uint32_t rn = n - (uint32_t)hn;
      uint8_t* in = (uint8_t*)malloc(rn ? rn : 1);
      uint8_t* out = (uint8_t*)malloc(us ? us : 1);
      memcpy(in, payload + hn, rn);
      bool ok = dcw::lz4_dec(in, rn, out, us, dict);
      if (ok == malformed || (ok && (us != explen || memcmp(out, want, us)))) {
        printf("rec %d: lz4_dec %s\n", rec, ok ? "WRONG/ACCEPTED" : "REFUSED");
        bad++;
      }
      free(in);
      free(out);
      if (rn <= DEC_MAX && us <= DEC_MAX) {
        for (int fill = 0; fill < 2; fill++) {
          uint8_t* li = (uint8_t*)malloc(DEC_MAX + DEC_PAD);
          uint8_t* lo = (uint8_t*)malloc(DEC_MAX + DEC_PAD);
          memset(li, fill ? 0xff : 0x00, DEC_MAX + DEC_PAD);
          memset(lo, 0xdd, DEC_MAX + DEC_PAD);
          memcpy(li, payload + hn, rn);
          bool okl = dcw::lz4_dec_lds(li, rn, lo, us, dict);
          if (okl == malformed || (okl && (us != explen || memcmp(lo, want, us)))) {
            printf("rec %d: lz4_dec_lds(fill %d) %s\n", rec, fill,
                   okl ? "WRONG/ACCEPTED" : "REFUSED");
            bad++;
          }
          free(li);
          free(lo);
        }
        lds_runs++;
      }
    }
    free(payload);
    free(want);
    refused += malformed;
    rec++;
  }
  fclose(f);
  free(dbuf);
  printf("lz4_dict_host: %d dictionaries, %d records (%d malformed, %d on the LDS "
         "form), %d failures\n", dicts, rec, refused, lds_runs, bad);
  if (bad == 0) printf("OK\n");
  return bad ? 1 : 0;
}
