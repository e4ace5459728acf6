// dzt_in_host — host check of the DZT input decoders, meant to be built
// with -fsanitize=address,undefined and run directly:
//   g++ -O1 -g -fsanitize=address,undefined -I toplingdb_amd/csrc \
//       tools/dzt_in_host/dzt_in_host.cpp toplingdb_amd/csrc/dcw_host.cpp \
//       oracle/liborc.so -l:libzstd.so.1 -Wl,-rpath,oracle -o dzt_in_host
//   ./dzt_in_host [corpus.bin]
// It compiles the SAME sources the GPU runs (dcw_dzt_dec.h: dzt_snap_dec,
// dzt_key_next) and the worker's DZT file parser (dcw_host.cpp: parse_dzt).
//  1. corpus file (written by tests/test_dzt_input_cpu.py), records:
//       'S' D:u32 n:u32 ulen:u32 dict stream expected[ulen]
//       'K' U:u32 ksize:u32 count:u32 block expected[count*(U+16)]
//       'F' size:u32 ok:u32 file
//     ulen / count == 0xffffffff: the decoder must refuse.
//  2. deterministic fuzz: random op streams of every form, then corrupted,
//     against oracle/liborc.so's orc_snappy_uncompress_dict — same
//     accept/reject decision, same bytes when accepted.
// Every buffer handed to a decoder is a heap allocation of the exact size,
// so a read or write one byte out of bounds stops the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dcw_dzt_dec.h"
#include "dcw_host.h"

extern "C" size_t orc_snappy_uncompress_dict(const uint8_t* dict, size_t D,
                                             const uint8_t* in, size_t n,
                                             uint8_t* out, size_t cap);

using namespace dcw;

static int g_fail = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      g_fail++;                       \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fprintf(stderr, "\n");          \
    }                                 \
  } while (0)

// exact-size heap copy (nullptr-free even for n == 0)
static uint8_t* dup_exact(const uint8_t* p, size_t n) {
  uint8_t* r = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(r, p, n);
  return r;
}

// decode through exact-size buffers; returns true + bytes on accept
static bool dec_exact(const std::vector<uint8_t>& dict,
                      const std::vector<uint8_t>& s, uint32_t cap,
                      std::vector<uint8_t>* out) {
  uint8_t* d = dup_exact(dict.data(), dict.size());
  uint8_t* in = dup_exact(s.data(), s.size());
  uint8_t* o = (uint8_t*)malloc(cap ? cap : 1);
  uint32_t got = 0;
  int rc = dzt_snap_dec(d, (uint32_t)dict.size(), in, (uint32_t)s.size(), o,
                        cap, &got);
  if (rc == DZT_OK) out->assign(o, o + got);
  free(d);
  free(in);
  free(o);
  return rc == DZT_OK;
}

// the kernel's walk over one key block (k_dzt_decode_keys)
static bool key_block(const uint8_t* blk, uint32_t ksize, uint32_t U,
                      uint32_t count, std::vector<uint8_t>* recs) {
  if (U > kDztUkeyMax || count > kDztKeysPerBlock) return false;
  uint8_t* kb = dup_exact(blk, ksize);
  uint8_t key[kDztUkeyMax] = {0};
  uint32_t pos = 0;
  uint64_t prev = 0;
  bool ok = true;
  for (uint32_t j = 0; j < count && ok; j++) {
    DztKeyRec r;
    ok = pos < ksize &&
         dzt_key_next(kb, ksize, &pos, U, j == 0, key, prev, &r) == DZT_OK;
    if (!ok) break;
    prev = r.tag;
    recs->insert(recs->end(), key, key + U);
    uint8_t t[16];
    memcpy(t, &r.tag, 8);
    memcpy(t + 8, &r.voff, 4);
    memcpy(t + 12, &r.vlen, 4);
    recs->insert(recs->end(), t, t + 16);
  }
  ok = ok && pos == ksize;
  free(kb);
  return ok;
}

static uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}

static void run_corpus(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    CHECK(false, "cannot open %s", path);
    return;
  }
  std::vector<uint8_t> buf;
  uint8_t tmp[65536];
  size_t g;
  while ((g = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + g);
  fclose(f);
  size_t p = 0, ns = 0, nk = 0, nf = 0, nrej = 0;
  while (p < buf.size()) {
    uint8_t kind = buf[p++];
    uint32_t a = rd32(&buf[p]), b = rd32(&buf[p + 4]), c = rd32(&buf[p + 8]);
    p += 12;
    if (kind == 'S') {
      std::vector<uint8_t> dict(buf.begin() + p, buf.begin() + p + a);
      p += a;
      std::vector<uint8_t> s(buf.begin() + p, buf.begin() + p + b);
      p += b;
      std::vector<uint8_t> out;
      if (c == 0xffffffffu) {
        // refused at any capacity the index could have promised
        CHECK(!dec_exact(dict, s, 16384, &out), "stream %zu accepted", ns);
        nrej++;
      } else {
        bool ok = dec_exact(dict, s, c, &out);
        CHECK(ok && out.size() == c && !memcmp(out.data(), &buf[p], c),
              "stream %zu wrong", ns);
        p += c;
      }
      ns++;
    } else if (kind == 'K') {
      std::vector<uint8_t> recs;
      bool ok = key_block(&buf[p], b, a, c == 0xffffffffu ? 64 : c, &recs);
      if (c == 0xffffffffu) {
        // with the count unknown: no count in 1..65 may be accepted
        for (uint32_t cnt = 1; cnt <= 65 && !ok; cnt++) {
          recs.clear();
          ok = key_block(&buf[p], b, a, cnt, &recs);
        }
        CHECK(!ok, "key block %zu accepted", nk);
        p += b;
        nrej++;
      } else {
        p += b;
        size_t want = (size_t)c * (a + 16);
        CHECK(ok && recs.size() == want && !memcmp(recs.data(), &buf[p], want),
              "key block %zu wrong", nk);
        p += want;
      }
      nk++;
    } else if (kind == 'F') {
      uint8_t* img = dup_exact(&buf[p], a);
      ParsedDzt z = parse_dzt(img, a);
      CHECK(z.ok == (b != 0), "file %zu: ok=%d want %u (%s)", nf, (int)z.ok, b,
            z.error.c_str());
      if (!z.ok) nrej++;
      free(img);
      p += a;
      nf++;
    } else {
      CHECK(false, "bad corpus record kind %u", kind);
      return;
    }
  }
  printf("corpus: %zu streams, %zu key blocks, %zu files (%zu refused)\n", ns,
         nk, nf, nrej);
}

// ---- fuzz ----
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 11);
}
static uint32_t rnd_in(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1); }

// random valid stream: ops of every form over dict || produced
static void gen_stream(const std::vector<uint8_t>& dict, uint32_t target,
                       std::vector<uint8_t>* s, std::vector<uint8_t>* raw) {
  std::vector<uint8_t> body;
  raw->clear();
  const uint32_t D = (uint32_t)dict.size();
  while (raw->size() < target) {
    uint32_t op = (uint32_t)raw->size();
    uint32_t k = rnd() % 8;
    if (k < 3 || op + D == 0) { // literal, 0..4 length bytes
      uint32_t ext = rnd() % 5;
      uint32_t len = ext == 0 ? rnd_in(1, 60) : rnd_in(1, ext == 1 ? 256 : 900);
      if (ext == 0) {
        body.push_back((uint8_t)((len - 1) << 2));
      } else {
        body.push_back((uint8_t)((59 + ext) << 2));
        for (uint32_t i = 0; i < ext; i++)
          body.push_back((uint8_t)((len - 1) >> (8 * i)));
      }
      for (uint32_t i = 0; i < len; i++) {
        uint8_t b = (uint8_t)(rnd() % 7 ? rnd() : 'a');
        body.push_back(b);
        raw->push_back(b);
      }
      continue;
    }
    // copy: pick where the source starts in dict || produced
    uint32_t offset;
    if (k == 3 && op) offset = rnd_in(1, op < 16 ? op : 16); // overlap range
    else if (k == 4 && D) offset = op + rnd_in(1, D);        // from the dict
    else if (k == 5 && D) offset = op + rnd_in(1, D < 24 ? D : 24); // dict tail
    else offset = rnd_in(1, op + D);
    uint32_t form = rnd() % 3 + 1, len;
    if (form == 1 && offset < 2048) {
      len = rnd_in(4, 11);
      body.push_back((uint8_t)(1 | ((len - 4) << 2) | ((offset >> 8) << 5)));
      body.push_back((uint8_t)offset);
    } else if (form != 3 && offset < 65536) {
      len = rnd_in(1, 64);
      body.push_back((uint8_t)(2 | ((len - 1) << 2)));
      body.push_back((uint8_t)offset);
      body.push_back((uint8_t)(offset >> 8));
    } else {
      len = rnd_in(1, 64);
      body.push_back((uint8_t)(3 | ((len - 1) << 2)));
      for (int i = 0; i < 4; i++) body.push_back((uint8_t)(offset >> (8 * i)));
    }
    for (uint32_t i = 0; i < len; i++) {
      uint32_t v = D + op + i - offset; // virtual position of the source
      raw->push_back(v < D ? dict[v] : (*raw)[v - D]);
    }
  }
  s->clear();
  uint8_t pre[5];
  int m = varint32_put(pre, (uint32_t)raw->size());
  s->insert(s->end(), pre, pre + m);
  s->insert(s->end(), body.begin(), body.end());
}

static void run_fuzz(int iters) {
  size_t accepted = 0, refused = 0;
  std::vector<uint8_t> dict, s, raw, mine, ref;
  for (int it = 0; it < iters; it++) {
    uint32_t D = it % 5 == 0 ? 0 : (it % 7 == 0 ? 49152 : rnd_in(1, 3000));
    dict.resize(D);
    for (auto& b : dict) b = (uint8_t)rnd();
    gen_stream(dict, rnd_in(1, it % 11 == 0 ? 20000 : 1500), &s, &raw);
    // valid stream: both accept, identical bytes
    const uint32_t cap = 32768;
    bool ok = dec_exact(dict, s, cap, &mine);
    CHECK(ok && mine == raw, "iter %d: valid stream refused or wrong", it);
    // corrupted variants
    for (int v = 0; v < 6; v++) {
      std::vector<uint8_t> t = s;
      uint32_t how = rnd() % 4;
      if (how == 0) t[rnd() % t.size()] ^= (uint8_t)(1u << (rnd() % 8));
      else if (how == 1) t.resize(rnd() % t.size() + 1); // truncate
      else if (how == 2) t[rnd() % t.size()] = (uint8_t)rnd();
      else { // 4-byte literal length near 2^32 spliced in
        uint32_t at = rnd() % t.size();
        uint8_t big[5] = {63 << 2, 0xfe, 0xff, 0xff, 0xff};
        t.insert(t.begin() + at, big, big + 5);
      }
      ref.assign(cap, 0);
      size_t r = orc_snappy_uncompress_dict(dict.data(), D, t.data(), t.size(),
                                            ref.data(), cap);
      bool mok = dec_exact(dict, t, cap, &mine);
      if (mok && mine.empty()) continue; // ulen 0: the reference's 0 is ambiguous
      bool rok = r != 0;
      CHECK(mok == rok, "iter %d/%d: accept mismatch mine=%d ref=%d", it, v,
            (int)mok, (int)rok);
      if (mok && rok)
        CHECK(mine.size() == r && !memcmp(mine.data(), ref.data(), r),
              "iter %d/%d: bytes differ", it, v);
      (mok ? accepted : refused)++;
    }
  }
  printf("fuzz: %d streams, corrupted variants: %zu accepted, %zu refused\n",
         iters, accepted, refused);
}

int main(int argc, char** argv) {
  crc32c_build_tables(&g_crc);
  if (argc > 1) run_corpus(argv[1]);
  run_fuzz(argc > 2 ? atoi(argv[2]) : 3000);
  if (g_fail) {
    printf("FAILED: %d\n", g_fail);
    return 1;
  }
  printf("OK\n");
  return 0;
}
