// host simulation of snap_dec_wave's batch/round structure vs oracle
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <random>
extern "C" {
  size_t orc_snappy_compress(const uint8_t*, size_t, uint8_t*);
  size_t orc_snappy_uncompress(const uint8_t*, size_t, uint8_t*, size_t);
}
#include "wave_sim.h"
int main(){
  std::mt19937 rng(19);
  for (int it = 0; it < 30000; it++) {
    int n = rng() % 4992 + 1;
    std::vector<uint8_t> d(n);
    int mode = it % 6;
    for (int i = 0; i < n; i++) {
      if (mode == 0) d[i] = rng();
      else if (mode == 1) d[i] = (i % (1 + it % 7));
      else if (mode == 2) d[i] = i >= 64 ? d[i-64] ^ (rng()%16==0) : rng();
      else if (mode == 3) d[i] = i >= 8 && rng()%8 ? d[i-8] : rng();
      else if (mode == 4) d[i] = i >= 2048 && rng()%4 ? d[i-2048] : (rng()%3==0 ? rng() : 'a');
      else d[i] = i >= 3 && rng()%5 ? d[i-3] : rng();   // offset-3 chains (round stress)
    }
    std::vector<uint8_t> enc(16 + n + n/6 + 1024);
    size_t en = orc_snappy_compress(d.data(), n, enc.data());
    std::vector<uint8_t> fast(n + 16), ref(n + 1);
    size_t rn = orc_snappy_uncompress(enc.data(), en, ref.data(), n);
    if (rn != (size_t)n) { printf("REF FAIL %d\n", it); return 1; }
    uint32_t fn = dec_wave_sim(enc.data(), (uint32_t)en, fast.data(), n);
    if (fn != (uint32_t)n || memcmp(fast.data(), d.data(), n)) {
      printf("WAVE MISMATCH it=%d mode=%d n=%d fn=%u\n", it, mode, n, fn); return 1; }
    std::vector<uint8_t> bad(enc.begin(), enc.begin()+en);
    bad[rng() % en] ^= 1 << (rng() % 8);
    std::vector<uint8_t> f2(n + 16), r2(n + 1);
    size_t a = orc_snappy_uncompress(bad.data(), en, r2.data(), n);
    uint32_t b = dec_wave_sim(bad.data(), (uint32_t)en, f2.data(), n);
    if ((a != 0) != (b != 0)) { printf("ACCEPT DISAGREE %d a=%zu b=%u\n", it, a, b); return 1; }
    if (a && memcmp(r2.data(), f2.data(), a)) { printf("CORRUPT DIFF %d\n", it); return 1; }
  }
  printf("wave fuzz OK\n");
  return 0;
}
