// gk_host — the general-key pieces that the dedup and DcwZipTable key-area
// kernels share with the host, driven on the CPU without a GPU job around
// them.  It compiles the kernels' own source: bound_cmp / rd_frag_upper
// (dcw_bound_cmp.h, what fsm_rd_covers runs) and the key-record writer
// (dcw_dzt_enc.h, what k_dzt_keys_g runs), plus fragment_tombstones and
// dzt_plan_files from dcw_host.cpp.
//
// Build: g++ -I toplingdb_amd/csrc tools/gk_host/gk_host.cpp
//            toplingdb_amd/csrc/dcw_host.cpp   (tests/test_genkeys_host_cpu.py)
//
// Usage: gk_host <job file> [<output file>]
// Job files are little-endian; str = u32 length + bytes.
//
// Fragment coverage:
//   "GKFR" | u32 general | u32 num_tombstones | (str start, str end, u64 seq)*
//   | u32 num_probes | (str user key)*
// The tombstones are fragmented as the worker does and laid out as dedup()
// uploads them (words, lengths, and with general != 0 the start bytes at
// DCW_GKEY_STRIDE).  For each probe prints the max seq of the fragment that
// contains it (0: none), found by rd_frag_upper with the arguments
// fsm_rd_covers passes: general != 0 gives the probe's side-table row and
// length (probes <= 48 bytes), general == 0 a null row (probes <= 16 bytes).
//
// Key area:
//   "GKKA" | u32 U | u64 target_file_size | u32 num_survivors
//   | (internal key of U+8 bytes, u32 value length)*
// Derives what the GPU hands the host (shared internal-key prefix, value
// length), plans the files (dzt_plan_files) and writes every key block in
// k_dzt_keys_g's schedule: one lane per record, record sizes, exclusive scan,
// dzt_krec_put from a DCW_GKEY_STRIDE side table, lane 0 the first internal
// key.  Writes to the output file
//   u32 num_files | (u64 len, key area bytes, u64 len, key index bytes)*
// with the key index laid out as build_dzt_file does.
// Both modes print "OK" last.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "dcw_bound_cmp.h"
#include "dcw_dzt_enc.h"
#include "dcw_host.h"

using namespace dcw;

namespace {

struct Reader {
  std::string buf;
  size_t at = 0;
  bool ok = true;
  const char* take(size_t n) {
    if (!ok || buf.size() - at < n) {
      ok = false;
      return nullptr;
    }
    const char* p = buf.data() + at;
    at += n;
    return p;
  }
  uint32_t u32() {
    uint32_t v = 0;
    if (const char* p = take(4)) memcpy(&v, p, 4);
    return v;
  }
  uint64_t u64() {
    uint64_t v = 0;
    if (const char* p = take(8)) memcpy(&v, p, 8);
    return v;
  }
  std::string bytes(size_t n) {
    const char* p = take(n);
    return p ? std::string(p, n) : std::string();
  }
  std::string str() { return bytes(u32()); }
};

int die(const char* msg) {
  fprintf(stderr, "gk_host: %s\n", msg);
  return 2;
}

int run_frags(Reader& r) {
  const bool general = r.u32() != 0;
  std::vector<SstTombstone> ts(r.u32());
  for (auto& t : ts) {
    t.start = r.str();
    t.end = r.str();
    t.seq = r.u64();
  }
  std::vector<std::string> probes(r.u32());
  for (auto& p : probes) p = r.str();
  if (!r.ok) return die("truncated job file");
  std::vector<TombstoneFragment> frags = fragment_tombstones(ts);
  // exact-size arrays, so a read past the last fragment is a sanitizer hit
  const uint32_t n = (uint32_t)frags.size();
  std::vector<uint64_t> k0(n), k1(n), seq(n);
  std::vector<uint32_t> len(n);
  std::vector<uint8_t> ext((size_t)n * DCW_GKEY_STRIDE);
  for (uint32_t i = 0; i < n; i++) {
    k0[i] = frags[i].k0;
    k1[i] = frags[i].k1;
    len[i] = frags[i].len;
    seq[i] = frags[i].max_seq;
    memcpy(ext.data() + (size_t)i * DCW_GKEY_STRIDE, frags[i].ext,
           DCW_GKEY_STRIDE);
  }
  for (auto& p : probes) {
    if (p.size() > (general ? (size_t)DCW_GKEY_MAX : 16u))
      return die("probe key longer than the mode's job keys");
    uint64_t a, b, c;
    make_normkey((const uint8_t*)p.data(), (uint32_t)p.size(), 0, &a, &b, &c);
    uint8_t row[DCW_GKEY_STRIDE] = {0}; // the probe's kext row
    memcpy(row, p.data(), p.size());
    uint32_t up = rd_frag_upper(k0.data(), k1.data(), len.data(),
                                general ? ext.data() : nullptr, n, a, b,
                                (uint32_t)p.size(), general ? row : nullptr);
    printf("%llu\n", (unsigned long long)(up ? seq[up - 1] : 0));
  }
  printf("OK\n");
  return 0;
}

int run_keyarea(Reader& r, const char* out_path) {
  const uint32_t U = r.u32();
  const uint64_t target = r.u64();
  const uint32_t n = r.u32();
  if (U < 1 || U > DCW_GKEY_MAX) return die("U outside 1..48");
  const uint32_t IK = U + 8;
  // the survivor arrays of the GPU job: side table, row index, tag, shared
  // internal-key prefix (k_shared_prefix), value length
  std::vector<uint8_t> kext((size_t)n * DCW_GKEY_STRIDE, 0);
  std::vector<uint32_t> s_w(n), vlen(n);
  std::vector<uint64_t> s_tag(n);
  std::vector<uint8_t> shared(n);
  std::string prev;
  for (uint32_t i = 0; i < n; i++) {
    std::string ik = r.bytes(IK);
    vlen[i] = r.u32();
    if (!r.ok) return die("truncated job file");
    s_w[i] = n - 1 - i; // rows out of order, as after a merge
    memcpy(kext.data() + (size_t)s_w[i] * DCW_GKEY_STRIDE, ik.data(), U);
    memcpy(&s_tag[i], ik.data() + U, 8);
    uint32_t s = 0;
    if (i > 0)
      while (s < IK && ik[s] == prev[s]) s++;
    shared[i] = (uint8_t)s;
    prev = ik;
  }
  std::vector<DztFilePlan> files =
      dzt_plan_files(vlen.data(), shared.data(), n, U, target);
  std::string out;
  uint32_t nf = (uint32_t)files.size();
  out.append((const char*)&nf, 4);
  for (auto& fp : files) {
    std::vector<uint8_t> keyarea(fp.key_area_size); // exact size
    std::vector<uint8_t> first_ikeys(fp.kbs.size() * (size_t)IK);
    for (size_t kb = 0; kb < fp.kbs.size(); kb++) {
      const DztKeyBlockPlan& K = fp.kbs[kb];
      if (K.count > kDztKB) return die("key block over 64 records");
      uint32_t sh[kDztKB], sz[kDztKB], off[kDztKB];
      for (uint32_t lane = 0; lane < K.count; lane++) {
        sh[lane] = dzt_krec_shared(shared[K.first + lane], U, lane == 0);
        sz[lane] = dzt_krec_size(sh[lane], U);
      }
      uint32_t run = 0; // what the wave's shuffle scan computes
      for (uint32_t lane = 0; lane < K.count; lane++) {
        off[lane] = run;
        run += sz[lane];
      }
      uint64_t kend = kb + 1 < fp.kbs.size() ? fp.kbs[kb + 1].koff
                                             : fp.key_area_size;
      if (K.koff + run != kend) return die("plan and record sizes disagree");
      for (uint32_t lane = 0; lane < K.count; lane++) {
        uint32_t e = K.first + lane;
        const uint8_t* ukey = kext.data() + (size_t)s_w[e] * DCW_GKEY_STRIDE;
        uint32_t wrote =
            dzt_krec_put(keyarea.data() + K.koff + off[lane], sh[lane], U, ukey,
                         s_tag[e], fp.voff[e - fp.first], vlen[e]);
        if (wrote != sz[lane]) return die("record size rule and writer disagree");
        if (lane == 0) {
          uint8_t* fk = first_ikeys.data() + kb * (size_t)IK;
          dzt_copy_bytes(fk, ukey, U);
          store64(fk + U, s_tag[e]);
        }
      }
    }
    std::string kindex;
    for (size_t kb = 0; kb < fp.kbs.size(); kb++) {
      kindex.append((const char*)first_ikeys.data() + kb * IK, IK);
      uint64_t koff = fp.kbs[kb].koff;
      uint64_t kend = kb + 1 < fp.kbs.size() ? fp.kbs[kb + 1].koff
                                             : fp.key_area_size;
      uint32_t ksize = (uint32_t)(kend - koff);
      uint64_t rank = fp.kbs[kb].first - fp.first;
      kindex.append((const char*)&koff, 8);
      kindex.append((const char*)&ksize, 4);
      kindex.append((const char*)&rank, 8);
    }
    uint64_t l = keyarea.size();
    out.append((const char*)&l, 8);
    out.append((const char*)keyarea.data(), keyarea.size());
    l = kindex.size();
    out.append((const char*)&l, 8);
    out.append(kindex);
  }
  std::ofstream of(out_path, std::ios::binary);
  of.write(out.data(), (std::streamsize)out.size());
  if (!of) return die("cannot write the output file");
  printf("files %u\nOK\n", nf);
  return 0;
}

} // namespace

int main(int argc, char** argv) {
  if (argc < 2) return die("usage: gk_host <job file> [<output file>]");
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) return die("cannot open the job file");
  Reader r;
  r.buf.assign(std::istreambuf_iterator<char>(in),
               std::istreambuf_iterator<char>());
  std::string magic = r.bytes(4);
  if (magic == "GKFR") return run_frags(r);
  if (magic == "GKKA") {
    if (argc < 3) return die("key-area mode needs an output file");
    return run_keyarea(r, argv[2]);
  }
  return die("bad magic");
}
