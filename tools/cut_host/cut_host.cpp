// cut_host — the worker's file cutter (FileCutter, dcw_host.h) driven on
// the CPU, without a GPU job around it.  Reads one job from a file, derives
// what the GPU would hand the host (per-survivor shared/klen/vlen and the
// grandparent positions), then loops as the worker's bbt_finish does: plan a
// chunk of blocks from the current position (plan_blocks, the host twin of
// k_plan_next), let FileCutter walk it, advance.  Output blocks are taken as
// uncompressed (csizes = unc_size), so jobs must use compression = 0.
//
// Build: g++ -I toplingdb_amd/csrc tools/cut_host/cut_host.cpp
//            toplingdb_amd/csrc/dcw_host.cpp   (tests/test_cut_cpu.py)
//
// Job file, little-endian:
//   "DCUT" | u64 target_file_size | u64 max_compaction_bytes
//   | u32 level_compaction_dynamic_file_size | u32 block_size
//   | u32 block_restart_interval | u32 block_size_deviation
//   | u32 num_grandparents | u32 num_survivors
//   | grandparents: (u32 len, smallest user key, u32 len, largest user key,
//                    u64 file_size)*
//   | survivors:    (u32 len, internal key, u32 value length)*
// Prints one line per output file,
//   file <first survivor> <entries> <rule> <partial_count>
// where rule says what ended the file (size, max_compaction_bytes, dynamic,
// or end for the last file) and partial_count is the cut's mid-block
// remainder, then "OK".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

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
  std::string str() {
    uint32_t n = u32();
    const char* p = take(n);
    return p ? std::string(p, n) : std::string();
  }
};

struct Grandparent {
  std::string smallest, largest;
  uint64_t file_size;
};

// The definition above k_gp_positions, on plain strings (std::string
// compares in raw bytewise order: bytes, then length): for user key u,
//   A(u) = #files with smallest <= u,
//   B(u) = #files with largest < u, plus the prefix of the files whose
//          largest == u and whose successor starts at that same key,
//   pos = A + B, nback = the length of that prefix.
void gp_positions(const std::vector<Grandparent>& gps,
                  const std::vector<std::string>& ikeys,
                  std::vector<uint32_t>* pos, std::vector<uint8_t>* nback) {
  size_t ng = gps.size();
  for (const std::string& ik : ikeys) {
    std::string u = ik.substr(0, ik.size() - 8);
    uint32_t A = 0, B = 0;
    while (A < ng && gps[A].smallest <= u) A++;
    while (B < ng && gps[B].largest < u) B++;
    uint32_t lb = B;
    while (B < ng && gps[B].largest == u && B + 1 < ng &&
           gps[B + 1].smallest == gps[B].largest)
      B++;
    uint32_t nb = B - lb;
    pos->push_back(A + B);
    nback->push_back((uint8_t)(nb > 255 ? 255 : nb));
  }
}

const char* rule_name(CutRule r) {
  switch (r) {
    case CutRule::kSize: return "size";
    case CutRule::kMaxCompactionBytes: return "max_compaction_bytes";
    case CutRule::kDynamic: return "dynamic";
    default: return "end";
  }
}

} // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: cut_host JOBFILE\n");
    return 2;
  }
  Reader r;
  {
    std::ifstream in(argv[1], std::ios::binary);
    r.buf.assign(std::istreambuf_iterator<char>(in),
                 std::istreambuf_iterator<char>());
  }
  const char* magic = r.take(4);
  if (!magic || memcmp(magic, "DCUT", 4) != 0) {
    fprintf(stderr, "cut_host: not a job file\n");
    return 2;
  }
  uint64_t target_file_size = r.u64();
  uint64_t max_compaction_bytes = r.u64();
  bool dynamic = r.u32() != 0;
  TableOpts o;
  o.block_size = r.u32();
  o.block_restart_interval = r.u32();
  o.block_size_deviation = r.u32();
  uint32_t ngp = r.u32(), nsurv = r.u32();
  std::vector<Grandparent> gps;
  std::vector<uint64_t> gp_sizes;
  for (uint32_t g = 0; g < ngp && r.ok; g++) {
    Grandparent gp;
    gp.smallest = r.str();
    gp.largest = r.str();
    gp.file_size = r.u64();
    gp_sizes.push_back(gp.file_size);
    gps.push_back(gp);
  }
  std::vector<std::string> ikeys;
  std::vector<uint8_t> shared, klen;
  std::vector<uint32_t> vlen;
  for (uint32_t i = 0; i < nsurv && r.ok; i++) {
    std::string k = r.str();
    vlen.push_back(r.u32());
    if (k.size() < 8 || k.size() > 255) r.ok = false;
    size_t sh = 0;
    if (i > 0) {
      const std::string& p = ikeys.back();
      while (sh < p.size() && sh < k.size() && p[sh] == k[sh]) sh++;
    }
    shared.push_back((uint8_t)sh);
    klen.push_back((uint8_t)k.size());
    ikeys.push_back(k);
  }
  if (!r.ok || r.at != r.buf.size()) {
    fprintf(stderr, "cut_host: malformed job file\n");
    return 2;
  }
  std::vector<uint32_t> gp_pos;
  std::vector<uint8_t> gp_nback;
  if (ngp) gp_positions(gps, ikeys, &gp_pos, &gp_nback);

  PlanIn in{shared.data(), klen.data(), vlen.data(), nsurv};
  FileCutter cutter(target_file_size, max_compaction_bytes, dynamic, ngp,
                    gp_pos.data(), gp_nback.data(), gp_sizes.data());
  size_t s = 0;
  while (s < nsurv) {
    size_t cur = s;
    uint64_t data_size = 0;
    FileCut fc;
    while (!fc.cut && cur < nsurv) {
      uint64_t want = target_file_size > data_size
                          ? target_file_size - data_size
                          : (64 << 10);
      std::vector<PlannedBlock> blocks =
          plan_blocks(in, cur, o, want + 2 * o.block_size);
      if (blocks.empty()) break;
      std::vector<uint32_t> csizes;
      for (auto& b : blocks) csizes.push_back(b.unc_size);
      fc = cutter.next_chunk(blocks, csizes, data_size, s, nsurv);
      for (size_t b = 0; b < fc.take; b++) data_size += csizes[b] + kTrailerSize;
      if (fc.take) cur = blocks[fc.take - 1].first + blocks[fc.take - 1].count;
      if (fc.take < blocks.size()) break;
    }
    if (fc.cut) cur = fc.cut_entry;
    if (cur == s) {
      fprintf(stderr, "cut_host: empty file at survivor %zu\n", s);
      return 1;
    }
    printf("file %zu %zu %s %u\n", s, cur - s, rule_name(fc.rule),
           fc.cut ? fc.partial_count : 0);
    s = cur;
  }
  printf("OK\n");
  return 0;
}
