// lz4_enc_host — the LZ4 output encoder (dcw_lz4_enc.h, the source
// k_compress_lz4 compiles) driven on the CPU in the kernel's schedule,
// without a GPU.  For every block of a corpus file, window by window, it
//   1. builds the u16 min-position table as the wave does, 64 lanes in a
//      shuffled order;
//   2. takes the 64 lane summaries (lz4_walk_segment<false>), joins them
//      with the seam scan in the kernel's log-step order (lz4_seam over
//      distances 1, 2, 4, ...), finds each lane's next lane with a match as
//      the ballot does, and places the lanes with an exclusive prefix sum of
//      lz4_lane_bytes;
//   3. after the ratio arithmetic on the measured total, repeats 1 and 2 and
//      emits (lz4_emit_lane, the first run's head, the carried-in literals,
//      at last the final sequence) in a shuffled lane order into a heap
//      buffer of EXACTLY preamble + total bytes: under AddressSanitizer a
//      write past what was measured is a heap overflow;
//   4. requires the payload to equal lz4_encode_block (the serial
//      restatement) and to decode back to the block through lz4_dec.
//
// Build: g++ -fsanitize=address,undefined -I toplingdb_amd/csrc
//            tools/lz4_enc_host/lz4_enc_host.cpp   (tests/test_lz4_output_cpu.py)
//
// usage: lz4_enc_host <corpus file> <streams file>
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

#include "dcw_lz4_dec.h"
#include "dcw_lz4_enc.h"

using namespace dcw;

namespace {

const uint32_t kLanes = 64;

struct Rng { // xorshift64*: the shuffles only need to differ per block
  uint64_t s;
  uint32_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return (uint32_t)((s * 0x2545F4914F6CDD1DULL) >> 32);
  }
};
void shuffled_lanes(Rng& r, uint32_t* order) {
  for (uint32_t i = 0; i < kLanes; i++) order[i] = i;
  for (uint32_t i = kLanes - 1; i > 0; i--) {
    uint32_t j = r.next() % (i + 1);
    uint32_t t = order[i];
    order[i] = order[j];
    order[j] = t;
  }
}

int fail(const std::string& name, const char* what) {
  printf("FAIL %s: %s\n", name.c_str(), what);
  return 1;
}

// what the wave knows about one window after the scan
struct Plan {
  uint16_t tab[1u << kSnapHashBits];
  Lz4Seg r[kLanes];
  uint32_t s0[kLanes], s1[kLanes], later[kLanes], lnext[kLanes],
      nibnext[kLanes], at[kLanes];
  uint64_t hasmask;
  uint32_t f0, l0, nib0, head_at, cin;
};

// steps 1 and 2; `carry` and `at` are the running literal count and output
// offset that pass from window to window
void plan_window(const uint8_t* in, uint32_t n, uint32_t base, uint32_t wend,
                 Rng& rng, uint32_t& carry, uint32_t& at, Plan& pl) {
  uint32_t order[kLanes];
  for (auto& t : pl.tab) t = 0xffffu;
  shuffled_lanes(rng, order);
  for (uint32_t k = 0; k < kLanes; k++)
    for (uint32_t p = base + order[k]; p + 4 <= wend; p += kLanes) {
      uint32_t h = (load32(in + p) * kSnapHashMul) >> (32 - kSnapHashBits);
      if (p - base < pl.tab[h]) pl.tab[h] = (uint16_t)(p - base);
    }
  uint32_t seg = (uint32_t)snap_segment_size(wend - base);
  Lz4Carry inc[kLanes];
  pl.hasmask = 0;
  for (uint32_t l = 0; l < kLanes; l++) {
    pl.s0[l] = wend - base > l * seg ? base + l * seg : wend;
    pl.s1[l] = wend - pl.s0[l] > seg ? pl.s0[l] + seg : wend;
    Lz4Seg none = {0, 0, 0, 0, 0};
    pl.r[l] = pl.s0[l] < wend ? lz4_walk_segment<false>(in, n, base, pl.s0[l],
                                                        pl.s1[l], pl.tab, nullptr)
                              : none;
    inc[l] = {pl.r[l].has, pl.r[l].trail};
    if (pl.r[l].has) pl.hasmask |= 1ull << l;
  }
  for (uint32_t sh = 1; sh < kLanes; sh <<= 1) { // the kernel's shfl_up steps
    Lz4Carry prev[kLanes];
    memcpy(prev, inc, sizeof(prev));
    for (uint32_t l = sh; l < kLanes; l++) inc[l] = lz4_seam(prev[l - sh], prev[l]);
  }
  uint32_t lrun[kLanes];
  for (uint32_t l = 0; l < kLanes; l++) {
    Lz4Carry ex = l ? inc[l - 1] : Lz4Carry{0, 0};
    lrun[l] = (ex.has ? ex.trail : carry + ex.trail) + pl.r[l].lead;
  }
  uint32_t total = 0;
  for (uint32_t l = 0; l < kLanes; l++) {
    uint64_t above = l == kLanes - 1 ? 0 : (pl.hasmask >> (l + 1)) << (l + 1);
    uint32_t nxt = above ? (uint32_t)__builtin_ctzll(above) : l;
    pl.later[l] = above != 0;
    pl.lnext[l] = lrun[nxt];
    pl.nibnext[l] = pl.r[nxt].nib;
    pl.at[l] = total; // exclusive prefix; rebased below
    total += lz4_lane_bytes(pl.r[l], pl.later[l], pl.lnext[l]);
  }
  pl.cin = carry;
  pl.head_at = at;
  if (pl.hasmask == 0) {
    carry += wend - base;
    return;
  }
  pl.f0 = (uint32_t)__builtin_ctzll(pl.hasmask);
  pl.l0 = lrun[pl.f0];
  pl.nib0 = pl.r[pl.f0].nib;
  uint32_t pre = 1 + lz4_ext_len(pl.l0) + carry;
  for (uint32_t l = 0; l < kLanes; l++) pl.at[l] += at + pre;
  at += pre + total;
  carry = inc[kLanes - 1].trail;
}

int run_block(const std::string& name, const uint8_t* in, uint32_t n, Rng& rng,
              std::ofstream& streams) {
  auto pl = std::make_unique<Plan>();
  // pass 1: measure
  uint32_t carry = 0, at = 0;
  for (uint32_t base = 0; base < n; base += kLz4Window)
    plan_window(in, n, base, n - base > kLz4Window ? base + kLz4Window : n, rng,
                carry, at, *pl);
  uint8_t hdr[5];
  uint32_t hl = (uint32_t)varint32_put(hdr, n);
  size_t cn = (size_t)hl + at + 1 + lz4_ext_len(carry) + carry;
  int accepted = cn <= (((uint64_t)896 * n) >> 10) ? 1 : 0;
  // pass 2: emit into exactly cn bytes (here also for a rejected block)
  std::unique_ptr<uint8_t[]> out(new uint8_t[cn]);
  memcpy(out.get(), hdr, hl);
  uint8_t* body = out.get() + hl;
  carry = at = 0;
  uint32_t order[kLanes];
  for (uint32_t base = 0; base < n; base += kLz4Window) {
    uint32_t wend = n - base > kLz4Window ? base + kLz4Window : n;
    plan_window(in, n, base, wend, rng, carry, at, *pl);
    if (pl->hasmask == 0) continue;
    shuffled_lanes(rng, order);
    for (uint32_t k = 0; k < kLanes; k++) {
      uint32_t l = order[k];
      if (l == pl->f0) {
        uint8_t* op = lz4_put_head(body + pl->head_at, pl->l0, pl->nib0);
        (void)lz4_copy(op, in + (base - pl->cin), pl->cin);
      }
      if (pl->s0[l] < wend)
        lz4_emit_lane(in, n, base, pl->s0[l], pl->s1[l], pl->tab, pl->r[l],
                      pl->later[l], pl->lnext[l], pl->nibnext[l],
                      body + pl->at[l]);
    }
  }
  uint8_t* op = lz4_put_head(body + at, carry, 0);
  op = lz4_copy(op, in + (n - carry), carry);
  if ((size_t)(op - out.get()) != cn) return fail(name, "emitted != measured");
  // references
  std::vector<uint8_t> ref(5 + lz4_max_compressed(n));
  size_t hn = lz4_encode_block(in, n, ref.data());
  if (hn != cn || memcmp(ref.data(), out.get(), cn) != 0)
    return fail(name, "kernel schedule != lz4_encode_block");
  std::unique_ptr<uint8_t[]> back(new uint8_t[n]);
  if (!lz4_dec(body, (uint32_t)(cn - hl), back.get(), n) ||
      memcmp(back.get(), in, n) != 0)
    return fail(name, "round trip through lz4_dec");
  uint32_t cn32 = (uint32_t)cn;
  streams.write((const char*)&cn32, 4);
  streams.write((const char*)out.get(), (std::streamsize)cn);
  printf("block %s %u %zu %d\n", name.c_str(), n, cn, accepted);
  return 0;
}

} // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: lz4_enc_host <corpus file> <streams file>\n");
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
  Rng rng{0x9E3779B97F4A7C15ULL};
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
    if (buf.size() - at < n || n == 0 || n > kLz4MaxUnc)
      return fail(name, "bad block length");
    // a heap copy of exactly n bytes: a read past the block is an overflow
    std::unique_ptr<uint8_t[]> in(new uint8_t[n]);
    memcpy(in.get(), buf.data() + at, n);
    at += n;
    if (run_block(name, in.get(), n, rng, streams) != 0) return 1;
    blocks++;
  }
  if (blocks == 0) return fail("corpus", "empty");
  streams.close();
  if (!streams) return fail("streams", "write failed");
  printf("OK\n");
  return 0;
}
