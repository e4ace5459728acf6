// dcw_host.h — PRODUCT host-side SST format logic: footer/index parsing of
// input SSTs, output meta tail (index/properties/metaindex/footer) assembly,
// the block/file plan FSM, and the synthetic-input generator.
//
// Byte format citations:
//  - block entries/restarts: table/block_based/block_builder.cc:21-32,128-253
//  - block footer u32:       table/block_based/data_block_footer.cc:24-39
//  - flush policy:           table/block_based/flush_block_policy.cc:37-71
//  - trailer:                block_based_table_builder.cc:1277-1330
//  - footer (53 B):          table/format.cc:191-259
//  - index:                  table/block_based/index_builder.{h,cc},
//                            format.cc IndexValue::EncodeTo
//  - properties/metaindex:   table/meta_blocks.cc
//  - file cutting:           db/compaction/compaction_outputs.cc:121-420
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "dcw_common.h"

namespace dcw {

extern Crc32cTables g_crc; // built in dcw_init / library load

struct TableOpts {
  uint32_t block_size = 4096;
  uint32_t block_restart_interval = 16;
  uint32_t index_block_restart_interval = 1;
  uint32_t format_version = 5;
  uint32_t checksum_type = 4; // kXXH3
  uint32_t compression = 0;
  uint64_t block_size_deviation = 10;
  std::string db_id, db_session_id, db_host_id;
  std::string cf_name = "default";
  uint32_t cf_id = 0;
  uint64_t orig_file_number = 0;
  uint64_t creation_time = 0;
  uint64_t file_creation_time = 0;
  uint64_t oldest_key_time = 0;
  int level_at_creation = 0;
  // bloom filter (FastLocalBloom): millibits/key, 0 = none
  uint32_t bloom_millibits_per_key = 0;
};

// ---- generic delta-encoded block builder (host-side blocks) ----
class BlockBuilder {
 public:
  BlockBuilder(uint32_t restart_interval, bool use_value_delta)
      : interval_(restart_interval), uvde_(use_value_delta) {
    restarts_.push_back(0);
  }
  void Add(const std::string& key, const std::string& value,
           const std::string* delta_value = nullptr);
  // AddWithLastKey semantics for table data blocks (external last key,
  // truncated to empty at block start — block_builder.cc:176-186)
  void AddWithLastKey(const uint8_t* key, size_t klen, const uint8_t* val,
                      size_t vlen, const uint8_t* last_key, size_t last_len);
  size_t CurrentSizeEstimate() const { return 8 + buf_.size() + 4 * (restarts_.size() - 1); }
  size_t EstimateSizeAfterKV(size_t klen, size_t vlen) const;
  bool empty() const { return buf_.empty(); }
  std::string Finish();
  void Reset() {
    buf_.clear();
    restarts_.assign(1, 0);
    counter_ = 0;
    last_key_.clear();
  }

 private:
  uint32_t interval_;
  bool uvde_;
  std::string buf_;
  std::vector<uint32_t> restarts_;
  uint32_t counter_ = 0;
  std::string last_key_;
};

// ---- input SST parsing ----
struct SstIndexEntry {
  uint64_t off, size; // BlockHandle of a data block
};
struct SstTombstone {
  std::string start, end; // user keys, [start, end)
  uint64_t seq = 0;
};
struct ParsedSst {
  uint32_t checksum_type = 4;
  std::vector<SstIndexEntry> data_blocks;
  std::vector<SstTombstone> tombstones; // "rocksdb.range_del" meta block
  std::string error;
  bool ok = false;
};
// Parses footer + index from an in-memory file image (host reads only the
// footer/index/meta regions; data block BYTES go to the GPU untouched).
ParsedSst parse_sst(const uint8_t* data, size_t size);

// ---- DcwZipTable ("DZT1") input parsing (format: oracle/dzt.c) ----
struct DztKeyIndexEntry {
  uint64_t koff;  // in the key area
  uint32_t ksize;
  uint64_t first_rank;
};
struct DztValueIndexEntry {
  uint64_t voff;  // in the value area
  uint32_t csize, ulen;
  uint64_t first_rank;
};
struct ParsedDzt {
  uint32_t checksum_type = 4;
  uint32_t ukey_len = 0;
  uint64_t n = 0, dict_size = 0;
  uint64_t dict_off = 0, value_off = 0, kindex_off = 0, vindex_off = 0;
  std::vector<DztKeyIndexEntry> kblocks;
  std::vector<DztValueIndexEntry> vblocks;
  uint64_t key_csum_usec = 0; // host time spent on the key-area checksum
  std::string error;
  bool ok = false;
};
// true when the image ends in the 96-byte DZT footer ("DCWZIP01")
bool is_dzt_file(const uint8_t* data, size_t size);
// Parses footer, props and both indexes; verifies the dict, key-index,
// value-index, props and key-area section checksums (value blocks carry
// their own trailers and are verified on the GPU); bounds-checks every
// index entry against its section.
ParsedDzt parse_dzt(const uint8_t* data, size_t size);

// ---- output meta tail ----
struct TailStats {
  uint64_t num_entries = 0, num_deletions = 0, num_merge_operands = 0;
  uint64_t num_range_deletions = 0;
  uint64_t raw_key_size = 0, raw_value_size = 0;
  uint64_t num_data_blocks = 0, data_size = 0;
};
// Builds everything after the data blocks: index block, properties,
// metaindex, footer.  separators[i] = index key for data block i (already
// shortened; last block's separator = its last key unshortened).
// sep_is_user_key: store separators without the 8-byte tag
// (props index_key_is_user_key) — valid when no adjacent blocks share a
// user key (index_builder.h:180-186).
std::string build_tail(const TableOpts& o, const TailStats& st,
                       const std::vector<SstIndexEntry>& handles,
                       const std::vector<std::string>& separators,
                       bool sep_is_user_key, uint64_t tail_start_offset,
                       const std::string& filter_content = std::string(),
                       uint64_t num_filter_entries = 0);

// write one block + 5-byte trailer to out; returns handle
SstIndexEntry append_block(std::string& out, const TableOpts& o,
                           const uint8_t* data, size_t n, bool try_compress);

// ---- plan FSM ----
struct PlanIn { // per-survivor metadata (D2H from the GPU)
  const uint8_t* shared;  // prefix shared with previous survivor (full ikey)
  const uint8_t* klen;    // internal key length
  const uint32_t* vlen;   // value length
  size_t n;
};
struct PlannedBlock {
  uint32_t first, count;   // survivor range
  uint32_t unc_size;       // uncompressed block size (with restarts+footer)
  uint32_t num_restarts;
};
// Pure block FSM (no file cuts): plan blocks from `from` until covering
// `min_bytes` of uncompressed output or entries run out.  If eoff_out is
// non-null it receives each planned entry's in-block byte offset (indexed
// from `from`), saving the emit path a second walk.
std::vector<PlannedBlock> plan_blocks(const PlanIn& in, size_t from,
                                      const TableOpts& o, uint64_t min_bytes,
                                      std::vector<uint32_t>* eoff_out = nullptr);

// ---- file cutting (ShouldStopBefore, compaction_outputs.cc:231-352) ----
// Decides where an output file ends, one call per emitted chunk of blocks.
// Without grandparents the file size only changes at block flushes, so the
// walk is block-level and the cut lands one entry after the crossing flush
// (the open block then holds exactly one entry).  With grandparents every
// entry is checked against the boundary-crossing rules and the cut may land
// mid-block.  The grandparent accounting (compaction_outputs.cc:121-230) is
// driven by per-survivor boundary positions precomputed on the GPU:
// gp_pos[i] = number of grandparent boundary points (smallest_0, largest_0,
// smallest_1, ...) "passed" by survivor i's user key under the reference's
// walk, gp_nback[i] = files before the current one whose largest equals the
// key (see k_gp_positions).  being_in_gap = pos is even.
enum class CutRule : uint8_t { kNone, kSize, kMaxCompactionBytes, kDynamic };
struct FileCut {
  bool cut = false;
  size_t take = 0;            // full blocks of the chunk that the file keeps
  uint64_t partial_first = 0; // mid-block remainder [partial_first, cut_entry)
  uint32_t partial_count = 0; // may be 0 (cut at a block boundary)
  uint64_t cut_entry = 0;     // first entry of the next file
  CutRule rule = CutRule::kNone; // which rule cut (reported by tools only)
};
class FileCutter {
 public:
  // One per job.  gp_pos / gp_nback are null when num_grandparents == 0 and
  // must outlive the cutter; gp_file_sizes has num_grandparents elements.
  FileCutter(uint64_t target_file_size, uint64_t max_compaction_bytes,
             bool level_compaction_dynamic_file_size,
             uint32_t num_grandparents, const uint32_t* gp_pos,
             const uint8_t* gp_nback, const uint64_t* gp_file_sizes);
  // blocks/csizes: the chunk just emitted, in order, continuing a file whose
  // data blocks so far take `data_size` bytes and whose first survivor is
  // `s`; nsurv = survivors of the job.
  FileCut next_chunk(const std::vector<PlannedBlock>& blocks,
                     const std::vector<uint32_t>& csizes, uint64_t data_size,
                     size_t s, size_t nsurv);

 private:
  // GetCurrentKeyGrandparentOverlappedBytes (compaction_outputs.cc:189-229)
  uint64_t gp_cur_overlap(uint64_t e) const;
  // UpdateGrandparentBoundaryInfo for entry e: returns the boundaries crossed
  uint64_t gp_update(uint64_t e);
  CutRule should_stop(uint64_t e, uint64_t off, uint64_t crossings,
                      uint64_t prev_overlapped) const;

  uint64_t target_, max_compaction_bytes_;
  bool dyn_;
  uint32_t ngp_;
  const uint32_t* gp_pos_;
  const uint8_t* gp_nback_;
  std::vector<uint64_t> gp_psum_; // prefix sums of the grandparent file sizes
  // Walk state.  It runs across the files of one job: only a cut resets
  // part of it (close-file resets, compaction_outputs.cc:374-380).
  bool seen_key_ = false;
  uint64_t last_pos_ = 0;
  uint64_t overlapped_ = 0; // grandparent_overlapped_bytes_
  uint64_t switched_ = 0;   // grandparent_boundary_switched_num_
};

// ---- range-tombstone fragments ----
// Fragment i covers user keys in [start_i, start_{i+1}); max_seq 0 marks a
// gap or the terminator.  Same construction as the oracle's rd_aggr,
// including the zero-seq gap/terminator fragments; sorted by start key in
// raw bytewise order.  Bounds may have any length: of a start key the device
// needs the prefix words, the true length and (general-key mode) the first
// DCW_GKEY_MAX bytes — see bound_cmp (dcw_bound_cmp.h).
struct TombstoneFragment {
  uint64_t k0, k1; // zero-padded big-endian start-key words
  uint32_t len;    // true byte length
  uint64_t max_seq;
  uint8_t ext[DCW_GKEY_STRIDE]; // first min(len, DCW_GKEY_MAX) bytes, 0-padded
};
std::vector<TombstoneFragment> fragment_tombstones(
    const std::vector<SstTombstone>& tombstones);

// ---- DcwZipTable ("DZT1") output plan ----
// Mirrors the oracle's DZT out_add/out_close rule (oracle/compact.c DZT
// branch; format: oracle/dzt.c): value blocks group greedily (<= 256 values,
// <= 16 KiB), a file is cut where an entry would open a new value block and
// the file's uncompressed bytes reached the target, key blocks hold 64.
enum : uint32_t {
  kDztKB = 64,
  kDztVbMax = 256,
  kDztVbUlenMax = 16384,
  kDztDictMax = 49152,
  kDztDictSampleBytes = 256,
};
struct DztValueBlockPlan {
  uint32_t first;     // survivor index of the block's first entry (absolute)
  uint32_t count;
  uint32_t ulen;      // uncompressed value bytes
  uint64_t stage_off; // offset in the file's value staging area
};
struct DztKeyBlockPlan {
  uint32_t first; // absolute survivor index
  uint32_t count; // <= kDztKB
  uint64_t koff;  // offset in the key area
};
struct DztFilePlan {
  uint64_t first = 0, count = 0; // survivor range
  std::vector<DztValueBlockPlan> vbs;
  std::vector<DztKeyBlockPlan> kbs;
  std::vector<uint32_t> voff; // per entry (file-local order): offset in its value block
  uint64_t key_area_size = 0;
  uint64_t raw_value = 0;
};
// vlen / shared: per-survivor value length and internal-key prefix shared
// with the previous survivor; U = the survivors' one user-key length
// (1..DCW_GKEY_MAX; the record size rule is dcw_dzt_enc.h's).
std::vector<DztFilePlan> dzt_plan_files(const uint32_t* vlen,
                                        const uint8_t* shared, size_t nsurv,
                                        uint32_t U, uint64_t target_file_size);

// ---- segmented file write ----
// Creates/truncates `path` and writes data[0, len) as up to max_segs
// segments of about seg_bytes each, one pwrite loop per segment on its own
// transient thread (the caller's thread writes the first).  tmpfs writes are
// page-clear + memcpy bound per thread.  Returns false on any failure.
bool write_file_segmented(const char* path, const uint8_t* data, size_t len,
                          size_t seg_bytes, size_t max_segs);

// ---- synthetic input generator (harness; the DB host's write path
//      stand-in, tools/db_bench_tool.cc:3468) ----
int gen_sst_file(const char* path, uint64_t seed, uint64_t num_entries,
                 uint32_t key_len, uint32_t value_len, uint64_t seq_base,
                 const TableOpts& opts);

// full streaming table writer (used by gen_sst_file and partial-block
// re-emission in the worker)
class TableWriter {
 public:
  explicit TableWriter(const TableOpts& o) : o_(o), data_block_(o.block_restart_interval, false) {}
  void Add(const uint8_t* ikey, size_t klen, const uint8_t* val, size_t vlen);
  std::string Finish(); // returns full file bytes
  uint64_t FileSize() const { return file_.size(); }
  const TailStats& stats() const { return st_; }

 private:
  void FlushData();
  void AddIndexEntry(const uint8_t* next_key, size_t next_len);
  TableOpts o_;
  BlockBuilder data_block_;
  std::string file_, last_key_;
  std::vector<SstIndexEntry> handles_;
  std::vector<std::string> separators_;
  bool sep_key_plus_seq_ = false;
  bool has_pending_ = false;
  SstIndexEntry pending_{};
  TailStats st_;
};

// FindShortestInternalKeySeparator (index_builder.cc:77-95 +
// util/comparator.cc:42-90); modifies start in place.
void shorten_separator(std::string& start, const uint8_t* limit, size_t limit_len);

} // namespace dcw
