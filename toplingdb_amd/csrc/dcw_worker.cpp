// dcw_worker.cpp — job orchestration + the C ABI (include/dcw.h).
//
// dcw_execute mirrors the worker side of ToplingDB's dcompact seam
// (CompactionExecutor::Execute, db/compaction/compaction_executor.h:165-171;
// worker lifecycle like DBImplSecondary::CompactWithoutInstallation,
// db/db_impl/db_impl_secondary.cc:805): deserialize job -> open input SSTs
// -> GPU hot loop (decode/merge/dedup/encode) -> write SSTs -> return file
// metas.  The hot path runs on the GPU (dcw_gpu.hip); the host does I/O,
// the block/file-cut plan FSM over per-entry size metadata
// (SURVEY.md §7 "plan pass"), and the per-file meta tail (<0.1% of bytes).
// There is NO CPU fallback: without a GPU, dcw_init fails.
#include <inttypes.h>
#include <sys/stat.h>

#include <cstdio>
#include <execinfo.h>
#include <fcntl.h>
#include <csignal>
#include <unistd.h>
#include <cstring>
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <future>
#include <thread>
#include <mutex>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dcw.h"
#include "dcw_gpu.h"
#include "dcw_host.h"

namespace dcw {
namespace {

std::mutex g_mu;
std::mutex g_out_mu; // guards out_files slots filled by tail threads

// Reusable GpuJob pool: device buffers are grow-only per job instance, so
// pooling keeps the no-hipMalloc-per-job property while allowing several
// jobs in flight on one device (the production dcompact worker runs
// concurrent jobs per node; per-job streams are non-blocking so pipelines
// interleave without cross-serialization).
// Fixed worker pool for per-file tail jobs (separators, meta tail, file
// write).  std::async spawns a fresh thread per task; at 10 jobs in
// flight that is hundreds of transient threads contending with the
// submission threads — a small fixed pool keeps host scheduling sane.
// Tail jobs never wait on other tail jobs (their nested pwrite segments
// use transient threads), so a bounded pool cannot deadlock.
struct TailPool {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::packaged_task<int()>> q;
  std::vector<std::thread> threads;
  bool started = false;
  void start_locked() {
    unsigned n = std::thread::hardware_concurrency();
    // 64 measured best at 10 jobs in flight on a 256-core box
    // (gpurun_out/hs_*.json sweep: 12.24 GB/s vs 11.67 at 32)
    unsigned workers = n ? (n < 64 ? n : 64) : 8;
    if (const char* e = getenv("DCW_TAIL_WORKERS")) {
      int w = atoi(e);
      if (w > 0 && w <= 256) workers = (unsigned)w;
    }
    for (unsigned i = 0; i < workers; i++)
      threads.emplace_back([this]() {
        for (;;) {
          std::packaged_task<int()> t;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [this]() { return !q.empty(); });
            t = std::move(q.front());
            q.pop_front();
          }
          t();
        }
      });
    for (auto& t : threads) t.detach();
    started = true;
  }
  std::future<int> submit(std::function<int()> fn) {
    std::packaged_task<int()> task(std::move(fn));
    std::future<int> f = task.get_future();
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!started) start_locked();
      q.push_back(std::move(task));
    }
    cv.notify_one();
    return f;
  }
};
// intentionally leaked: destroying the pool's mutex/condvar at process
// exit while detached workers wait on them hangs exit (pthread_cond
// destruction blocks with waiters)
TailPool& tails() {
  static TailPool* p = new TailPool;
  return *p;
}

struct JobPool {
  std::mutex mu;
  std::vector<GpuJob*> free_jobs;
  GpuJob* acquire() {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!free_jobs.empty()) {
        GpuJob* j = free_jobs.back();
        free_jobs.pop_back();
        return j;
      }
    }
    if (getenv("DCW_PHASE_DEBUG"))
      fprintf(stderr, "[pool] miss -> new GpuJob\n");
    return new GpuJob();
  }
  void put(GpuJob* j) {
    std::lock_guard<std::mutex> lk(mu);
    free_jobs.push_back(j);
  }
} g_jobs;
bool g_inited = false;
uint64_t g_next_stage_handle = 1;

struct StagedJob {
  StagedInput dev;
  uint64_t in_bytes = 0;
  std::vector<SstTombstone> tombstones;
};
std::unordered_map<uint64_t, StagedJob*> g_staged;
std::mutex g_cancel_mu;
std::set<int32_t> g_cancelled;

bool consume_cancel(int32_t job_id) {
  std::lock_guard<std::mutex> lk(g_cancel_mu);
  return g_cancelled.erase(job_id) != 0;
}
bool peek_cancel(int32_t job_id) {
  std::lock_guard<std::mutex> lk(g_cancel_mu);
  return g_cancelled.count(job_id) != 0;
}

uint64_t now_usec() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (uint64_t)ts.tv_sec * 1000000 + ts.tv_nsec / 1000;
}

struct LoadedInputs; // fwd (RawBuf defined below the pin pool)
int load_inputs(const dcw_job_desc* d, LoadedInputs* L, std::string* err,
                GpuJob* job = nullptr);

TableOpts opts_from_desc(const dcw_job_desc* d) {
  TableOpts o;
  if (d->block_size) o.block_size = d->block_size;
  if (d->block_restart_interval) o.block_restart_interval = d->block_restart_interval;
  if (d->index_block_restart_interval)
    o.index_block_restart_interval = d->index_block_restart_interval;
  if (d->format_version) o.format_version = d->format_version;
  o.checksum_type = d->checksum_type;
  o.compression = d->compression;
  if (d->block_size_deviation) o.block_size_deviation = d->block_size_deviation;
  o.db_id = d->db_id ? d->db_id : "";
  o.db_session_id = d->db_session_id ? d->db_session_id : "";
  o.db_host_id = d->db_host_id ? d->db_host_id : "";
  o.cf_name = d->cf_name ? d->cf_name : "default";
  o.cf_id = d->cf_id;
  o.creation_time = d->oldest_ancester_time ? d->oldest_ancester_time : d->current_time;
  o.file_creation_time = d->current_time;
  o.oldest_key_time = 0;
  o.level_at_creation = d->output_level;
  o.bloom_millibits_per_key = d->bloom_millibits_per_key;
  return o;
}

// Pinned (hipHostMalloc) buffer pool for output file images: D2H into
// pageable memory runs at ~9 GB/s, pinned at PCIe rate; buffers are
// recycled across files/steps so the pin cost is paid once.
#include <hip/hip_runtime.h>
struct PinPool {
  std::mutex mu;
  std::vector<std::pair<uint8_t*, size_t>> free_bufs;
  uint8_t* acquire(size_t n, size_t* cap) {
    {
      // best fit: input blobs (~600 MB) and output images (~70 MB) share
      // this pool; first-fit would hand a blob-sized buffer to an image
      // and force a fresh pin for the next blob
      std::lock_guard<std::mutex> lk(mu);
      size_t best = free_bufs.size();
      for (size_t i = 0; i < free_bufs.size(); i++)
        if (free_bufs[i].second >= n &&
            (best == free_bufs.size() || free_bufs[i].second < free_bufs[best].second))
          best = i;
      if (best < free_bufs.size()) {
        auto b = free_bufs[best];
        free_bufs.erase(free_bufs.begin() + best);
        *cap = b.second;
        return b.first;
      }
    }
    size_t c = n + n / 8 + (1 << 20);
    uint8_t* p = nullptr;
    if (hipHostMalloc((void**)&p, c, hipHostMallocDefault) != hipSuccess) {
      p = (uint8_t*)malloc(c); // fall back to pageable (still correct)
    }
    *cap = c;
    return p;
  }
  void release(uint8_t* p, size_t cap) {
    std::lock_guard<std::mutex> lk(mu);
    free_bufs.emplace_back(p, cap);
  }
  void drain() {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& b : free_bufs) (void)hipHostFree(b.first);
    free_bufs.clear();
  }
};
PinPool g_pin_pool;

// grow-without-zero-fill byte buffer backed by the pinned pool
struct RawBuf {
  uint8_t* p = nullptr;
  size_t len = 0, cap = 0;
  void reserve(size_t n) {
    if (cap >= n) return;
    size_t ncap = 0;
    uint8_t* np = g_pin_pool.acquire(n + n / 4, &ncap);
    if (p) {
      memcpy(np, p, len);
      g_pin_pool.release(p, cap);
    }
    p = np;
    cap = ncap;
  }
  void resize_uninit(size_t n) {
    reserve(n);
    len = n;
  }
  void append(const void* src, size_t n) {
    reserve(len + n);
    memcpy(p + len, src, n);
    len += n;
  }
  void release() { p = nullptr; len = cap = 0; }
  void swap(RawBuf& o) {
    std::swap(p, o.p);
    std::swap(len, o.len);
    std::swap(cap, o.cap);
  }
  ~RawBuf() {
    if (p) g_pin_pool.release(p, cap);
  }
};

// Input images live in PINNED memory (RawBuf over the pin pool): the
// per-job H2D of ~600 MB runs at PCIe rate and overlaps other jobs'
// kernels on this job's own stream.  A real dcompact worker pays this
// read+upload for every job (the reference hot loop reads its inputs,
// table/block_fetcher.cc:242), so the bench times it by default.
struct LoadedInputs {
  RawBuf blob; // all files concatenated (pinned)
  GpuInputs gi;
  uint64_t in_bytes = 0;
  std::vector<SstTombstone> tombstones; // all inputs' range deletions
  bool host_decoded = false; // zstd inputs were rewritten (see below)
  // sub-phase wall attribution (printed under DCW_PHASE_DEBUG)
  uint64_t us_reserve = 0, us_pread = 0, us_parse = 0, us_stage = 0;
  uint64_t us_dzt_keycsum = 0; // part of us_parse: DZT key-area checksums
};

// minimal libzstd ABI (runtime lib only in this image); the worker only
// DECODES zstd inputs — SURVEY §8f-1's input side.  The GPU codec stays
// snappy; zstd blocks are decoded host-side at load and handed to the
// device as raw blocks with recomputed trailers.
extern "C" size_t ZSTD_decompress(void*, size_t, const void*, size_t);
extern "C" unsigned ZSTD_isError(size_t);

int load_inputs(const dcw_job_desc* d, LoadedInputs* L, std::string* err,
                GpuJob* job) {
  // pre-size the pinned blob so reads land in place (no regrow memcpy)
  uint64_t total = 0;
  for (uint32_t r = 0; r < d->num_runs; r++)
    for (uint32_t f = 0; f < d->runs[r].num_files; f++) {
      struct stat st;
      if (stat(d->runs[r].files[f], &st) != 0) {
        *err = std::string("cannot stat ") + d->runs[r].files[f];
        return -1;
      }
      total += (uint64_t)st.st_size;
    }
  uint64_t tphase = now_usec();
  L->blob.reserve(total);
  L->us_reserve += now_usec() - tphase;
  tphase = now_usec();
  // overlap H2D with the remaining file reads: each file's bytes start
  // streaming to the device the moment its read completes
  if (job && job->stage_begin(total, err) != 0) return -1;
  L->us_stage += now_usec() - tphase;
  L->gi.run_block_begin.push_back(0);
  uint32_t cstype = 0xffffffff;
  for (uint32_t r = 0; r < d->num_runs; r++) {
    for (uint32_t f = 0; f < d->runs[r].num_files; f++) {
      const char* path = d->runs[r].files[f];
      int fd = open(path, O_RDONLY);
      if (fd < 0) {
        *err = std::string("cannot open ") + path;
        return -1;
      }
      struct stat st;
      if (fstat(fd, &st) != 0) {
        close(fd);
        *err = std::string("cannot stat ") + path;
        return -1;
      }
      uint64_t sz = (uint64_t)st.st_size;
      uint64_t base = L->blob.len;
      uint64_t tf = now_usec();
      L->blob.reserve(base + sz);
      L->us_reserve += now_usec() - tf;
      tf = now_usec();
      // segmented parallel read: a single-thread fread of a ~64 MiB SST is
      // ~10 GB/s and sits on the job's critical path (the write side is
      // already segmented)
      uint8_t* dstp = L->blob.p + base;
      static const uint64_t max_seg = [] {
        const char* e = getenv("DCW_READ_SEGS");
        int v = e ? atoi(e) : 4;
        return (uint64_t)(v > 0 && v <= 16 ? v : 4);
      }();
      const uint64_t kSeg = 16u << 20;
      uint64_t nseg = (sz + kSeg - 1) / kSeg;
      if (nseg > max_seg) nseg = max_seg;
      if (nseg == 0) nseg = 1;
      uint64_t seg = (sz + nseg - 1) / nseg;
      std::vector<std::future<bool>> segr;
      for (uint64_t si = 1; si < nseg; si++) {
        uint64_t off = si * seg;
        uint64_t cnt = off < sz ? std::min(seg, sz - off) : 0;
        segr.emplace_back(std::async(std::launch::async, [fd, dstp, off, cnt]() {
          uint64_t done = 0;
          while (done < cnt) {
            ssize_t g = pread(fd, dstp + off + done, cnt - done,
                              (off_t)(off + done));
            if (g <= 0) return false;
            done += (uint64_t)g;
          }
          return true;
        }));
      }
      bool ok = true;
      {
        uint64_t cnt = std::min(seg, sz);
        uint64_t done = 0;
        while (done < cnt) {
          ssize_t g = pread(fd, dstp + done, cnt - done, (off_t)done);
          if (g <= 0) {
            ok = false;
            break;
          }
          done += (uint64_t)g;
        }
      }
      for (auto& fw : segr) ok = fw.get() && ok;
      close(fd);
      if (!ok) {
        *err = std::string("short read ") + path;
        return -1;
      }
      L->blob.len = base + sz;
      L->us_pread += now_usec() - tf;
      tf = now_usec();
      if (job && job->stage_chunk(base, L->blob.p + base, sz, err) != 0)
        return -1;
      L->us_stage += now_usec() - tf;
      tf = now_usec();
      if (is_dzt_file(L->blob.p + base, sz)) {
        // DcwZipTable input: the tables go to the GPU job beside the
        // BlockBasedTable block list, placed by blocks_before
        ParsedDzt pz = parse_dzt(L->blob.p + base, sz);
        L->us_parse += now_usec() - tf;
        L->us_dzt_keycsum += pz.key_csum_usec;
        if (!pz.ok) {
          *err = std::string(path) + ": " + pz.error;
          return -1;
        }
        if (cstype == 0xffffffff) cstype = pz.checksum_type;
        if (cstype != pz.checksum_type) {
          *err = "mixed input checksum types unsupported";
          return -1;
        }
        DztFileRef zf;
        zf.run = r;
        zf.blocks_before = (uint32_t)L->gi.blocks.size();
        zf.ukey_len = pz.ukey_len;
        zf.dict_size = (uint32_t)pz.dict_size;
        zf.n = pz.n;
        zf.key_off = base;
        zf.dict_off = base + pz.dict_off;
        zf.value_off = base + pz.value_off;
        zf.kindex_off = base + pz.kindex_off;
        zf.kblocks = std::move(pz.kblocks);
        zf.vblocks = std::move(pz.vblocks);
        L->gi.dzt_files.push_back(std::move(zf));
        L->in_bytes += sz;
        continue;
      }
      ParsedSst ps = parse_sst(L->blob.p + base, sz);
      L->us_parse += now_usec() - tf;
      if (!ps.ok) {
        *err = std::string(path) + ": " + ps.error;
        return -1;
      }
      if (cstype == 0xffffffff) cstype = ps.checksum_type;
      if (cstype != ps.checksum_type) {
        *err = "mixed input checksum types unsupported";
        return -1;
      }
      for (auto& h : ps.data_blocks)
        L->gi.blocks.push_back({base + h.off, (uint32_t)h.size});
      for (auto& t : ps.tombstones) L->tombstones.push_back(t);
      L->in_bytes += sz;
    }
    L->gi.run_block_begin.push_back((uint32_t)L->gi.blocks.size());
  }
  // zstd input blocks (type byte 0x7 in the trailer): verify + decode on
  // the host, rebuild the staged blob with raw blocks + recomputed
  // trailers (decompression output is unique, so parity is unaffected;
  // the reference reads its inputs through the same libzstd,
  // util/compression.h ZSTD_Uncompress)
  bool any_zstd = false;
  uint32_t ct = cstype == 0xffffffff ? 4 : cstype;
  tphase = now_usec();
  for (auto& blk : L->gi.blocks)
    if (L->blob.p[blk.off + blk.size] == 7) {
      any_zstd = true;
      break;
    }
  L->us_parse += now_usec() - tphase;
  if (any_zstd && !L->gi.dzt_files.empty()) {
    // the rewrite below rebuilds the blob from BlockBasedTable blocks alone
    *err = "zstd BlockBasedTable inputs cannot be combined with DZT inputs";
    return -1;
  }
  if (any_zstd) {
    if (job) { // already-streamed chunks are superseded by a full restage
      job->stage_cancel();
    }
    RawBuf nb;
    uint64_t est = L->blob.len * 2 + (16u << 20);
    nb.reserve(est);
    for (auto& blk : L->gi.blocks) {
      const uint8_t* body = L->blob.p + blk.off;
      uint8_t type = body[blk.size];
      uint64_t noff = nb.len;
      if (type == 7) {
        uint32_t stored;
        memcpy(&stored, body + blk.size + 1, 4);
        if (ct != 0 &&
            stored != block_checksum(ct, &g_crc, body, blk.size, type)) {
          *err = "zstd input block checksum mismatch";
          return -1;
        }
        uint32_t un;
        int hn = varint32_get(body, body + (blk.size < 5 ? blk.size : 5), &un);
        if (hn < 0) {
          *err = "bad zstd preamble in input block";
          return -1;
        }
        nb.reserve(nb.len + un + 8);
        size_t got = ZSTD_decompress(nb.p + nb.len, un, body + hn,
                                     blk.size - hn);
        if (ZSTD_isError(got) || got != un) {
          *err = "zstd input block corrupt";
          return -1;
        }
        nb.len += un;
        uint8_t tr[5];
        tr[0] = 0;
        uint32_t cs = block_checksum(ct, &g_crc, nb.p + noff, un, 0);
        memcpy(tr + 1, &cs, 4);
        nb.append(tr, 5);
        blk.off = noff;
        blk.size = un;
      } else {
        nb.append(body, blk.size + 5);
        blk.off = noff;
      }
    }
    L->blob.swap(nb); // nb's dtor returns the old blob to the pool
    L->host_decoded = true;
  }
  L->gi.blob = L->blob.p;
  L->gi.blob_size = L->blob.len;
  L->gi.checksum_type = ct;
  return 0;
}

// fixed-size block boundary key (ikey <= 24 B in the worker envelope);
// avoids per-block heap strings on the main thread
struct BKey {
  uint8_t len = 0;
  char b[72]; // internal key <= 56 B (general-key envelope)
};

int fail(dcw_job_result* res, int code, const std::string& msg) {
  res->status = code;
  snprintf(res->error, sizeof(res->error), "%s", msg.c_str());
  return code;
}

// fine-grained wall attribution (DCW_PHASE_DEBUG=1 prints at job end)
enum WallSlot {
  kWpLoad, kWpStage, kWpDecode, kWpMerge, kWpDedup, kWpPlan, kWpEmit,
  kWpWalkPack, kWpGather, kWpTailSpawn, kWpJoin, kWpOther, kWpChainWalk,
  kWpSlots
};
struct WallProf {
  const char* names[kWpSlots] = {"load",  "stage", "decode", "merge",
                                 "dedup", "plan",  "emit",   "walkpack",
                                 "gather", "tailspawn", "join", "other",
                                 "chainwalk"};
  uint64_t us[kWpSlots] = {0};
  uint64_t t_last = 0;
  void mark(WallSlot slot) {
    uint64_t now = now_usec();
    us[slot] += now - t_last;
    t_last = now;
  }
};

// What the steps of one dcw_execute call share.
struct JobCtx {
  const dcw_job_desc* d;
  dcw_job_result* res;
  GpuJob& job;
  uint64_t t_start;
  WallProf wp;
  uint64_t us_reset = 0;
  // inputs: exactly one of flush_mode / staged / L is in use
  bool flush_mode = false;
  StagedJob* staged = nullptr;
  LoadedInputs L;
  uint64_t in_bytes = 0;
  const std::vector<SstTombstone>* tombstones = nullptr;
  std::vector<GpuJob::RdFrag> rd_frags;
};

// ---- dcw_execute steps: check -> acquire -> front -> finish ----
int check_desc(const dcw_job_desc* d, dcw_job_result* res) {
  if (!g_inited)
    return fail(res, 10, "dcw_init not called or no gfx950 device (no CPU fallback)");
  if (d->struct_size != sizeof(dcw_job_desc))
    return fail(res, 11, "ABI mismatch: dcw_job_desc size");
  if (d->comparator_name &&
      strcmp(d->comparator_name, "leveldb.BytewiseComparator") != 0)
    return fail(res, 12, "unsupported comparator (bytewise only)");
  if (d->compression > 1)
    return fail(res, 13, "unsupported compression (none/snappy only)");
  if (d->checksum_type != 0 && d->checksum_type != 1 && d->checksum_type != 4)
    return fail(res, 14,
                "unsupported checksum_type (kNoChecksum/kCRC32c/kXXH3 only)");
  if (d->output_table_factory > 1)
    return fail(res, 14, "unsupported output_table_factory");
  return 0;
}

// read + parse inputs (host I/O), or pick up what is already there
int acquire_inputs(JobCtx& c) {
  const dcw_job_desc* d = c.d;
  c.flush_mode = d->flush_kv != nullptr;
  if (c.flush_mode) {
    // flush offload: the input is one sorted raw-KV
    // memtable stream; semantically a single-run compaction at L0
    if (d->num_runs || d->staged_handle)
      return fail(c.res, 14, "flush job must carry no SST runs");
    if (d->flush_num_entries == 0 || !d->flush_offsets)
      return fail(c.res, 14, "empty flush job");
    c.in_bytes = d->flush_kv_bytes;
  } else if (d->staged_handle) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_staged.find(d->staged_handle);
    if (it == g_staged.end()) return fail(c.res, 15, "bad staged handle");
    c.staged = it->second;
    c.in_bytes = c.staged->in_bytes;
    c.tombstones = &c.staged->tombstones;
  } else {
    std::string err;
    if (load_inputs(d, &c.L, &err, &c.job) != 0) return fail(c.res, 16, err);
    c.wp.mark(kWpLoad);
    c.in_bytes = c.L.in_bytes;
    c.tombstones = &c.L.tombstones;
  }
  // range deletions: supported envelope only (mirrors oracle/compact.c
  // rd_aggr — bottommost, no snapshots, no grandparents; all tombstones
  // are then obsolete at emission and only drop covered point keys)
  if (c.tombstones && !c.tombstones->empty()) {
    if (!d->bottommost_level || d->num_snapshots || d->num_grandparents)
      return fail(c.res, 29,
                  "range deletions outside supported envelope "
                  "(bottommost, no snapshots, no grandparents)");
    for (auto& f : fragment_tombstones(*c.tombstones)) {
      GpuJob::RdFrag r{f.k0, f.k1, f.len, f.max_seq, {0}};
      memcpy(r.ext, f.ext, sizeof(r.ext));
      c.rd_frags.push_back(r);
    }
  }
  return 0;
}

// GPU front half: stage, decode, merge, dedup
int run_front(JobCtx& c) {
  const dcw_job_desc* d = c.d;
  GpuJob& job = c.job;
  std::string err;
  if (c.flush_mode) {
    if (consume_cancel(d->job_id))
      return fail(c.res, 30 /*DCW_CANCELLED*/, "job cancelled");
    if (job.decode_flush(d, &err) != 0) return fail(c.res, 18, err);
    c.wp.mark(kWpDecode);
  } else if (c.staged) {
    if (job.stage_adopt(c.staged->dev, &err) != 0) return fail(c.res, 17, err);
    c.wp.mark(kWpStage);
  } else {
    if (job.stage(c.L.gi, &err) != 0) return fail(c.res, 17, err);
  }
  if (!c.flush_mode) {
    if (consume_cancel(d->job_id))
      return fail(c.res, 30 /*DCW_CANCELLED*/, "job cancelled");
    if (job.decode(&err) != 0) return fail(c.res, 18, err);
    c.wp.mark(kWpDecode);
  }
  if (job.general_keys) {
    // general-key mode envelope: this combination still falls back local.
    // (DcwZipTable output needs one user-key length over the SURVIVORS,
    // which only dedup knows: dzt_finish checks it.)
    if (d->num_grandparents > 0)
      return fail(c.res, 29, "grandparent cutting with general-shape keys "
                             "outside envelope");
  }
  if (job.merge(&err) != 0) return fail(c.res, 19, err);
  c.wp.mark(kWpMerge);
  job.set_range_del_frags(c.rd_frags);
  if (job.dedup(d, &err) != 0) return fail(c.res, 20, err);
  c.wp.mark(kWpDedup);
  return 0;
}

// the part of the result that both output paths fill the same way
void fill_result(JobCtx& c, const std::vector<dcw_output_file>& out_files,
                 uint64_t out_bytes, uint64_t out_entries) {
  dcw_job_result* res = c.res;
  res->num_files = (uint32_t)out_files.size();
  res->files =
      (dcw_output_file*)malloc(sizeof(dcw_output_file) * (out_files.size() + 1));
  memcpy(res->files, out_files.data(),
         sizeof(dcw_output_file) * out_files.size());
  res->in_bytes = c.in_bytes;
  res->out_bytes = out_bytes;
  res->in_entries = c.job.num_input_entries();
  res->out_entries = out_entries;
  res->t_h2d_usec = (uint64_t)(c.job.ms_h2d * 1000);
  res->t_gpu_usec = (uint64_t)((c.job.ms_decode + c.job.ms_merge +
                                c.job.ms_dedup + c.job.ms_emit) * 1000);
  res->work_time_usec = now_usec() - c.t_start;
  res->status = 0;
}

std::string output_path(const dcw_job_desc* d, uint64_t file_number) {
  char path[600];
  snprintf(path, sizeof(path), "%s/%06" PRIu64 ".sst", d->output_dir,
           file_number);
  return path;
}

// ---- BlockBasedTable output path ----
// One output file: filled by the main thread while the file's blocks are
// emitted, then handed whole to a tail thread (finish_bbt_file).
struct BbtOutputs {
  std::vector<dcw_output_file> files; // slots are written by tail threads
  uint64_t total_bytes = 0;           // under g_out_mu, like the slots
};
struct TailJob {
  TableOpts o;
  RawBuf image; // data-block region accumulated on host
  // output D2H transfers land in `image` asynchronously (second HIP
  // stream); every reader of image bytes waits these events first
  std::vector<void*> pend;
  std::vector<SstIndexEntry> handles;
  std::vector<BKey> first_keys, last_keys;
  uint64_t file_first = 0, file_count = 0;
  uint64_t mn_seq = ~0ull, mx_seq = 0, n_tomb = 0; // file seq stats
  std::string path;
  std::string filter_content;
  uint64_t n_filter = 0;
  // per-survivor lengths of the job, and where the file's meta goes
  const uint8_t* klen = nullptr;
  const uint32_t* vlen = nullptr;
  BbtOutputs* out = nullptr;
  size_t slot = 0;

  // settle in-flight D2H before `image` grows past its capacity: realloc
  // would memcpy regions still being written (rare: image is pre-reserved)
  void settle_before_growth(size_t new_len) {
    if (new_len <= image.cap) return;
    for (void* e : pend) GpuJob::wait_event(e);
    pend.clear();
  }
  void add_seq(uint64_t mn, uint64_t mx, uint64_t tomb) {
    if (mn < mn_seq) mn_seq = mn;
    if (mx > mx_seq) mx_seq = mx;
    n_tomb += tomb;
  }
};

// Runs on a tail thread: separators, meta tail, file write, result slot.
int finish_bbt_file(TailJob& tj) {
  for (void* e : tj.pend) GpuJob::wait_event(e); // image bytes complete
  // separators (FindShortestInternalKeySeparator between adjacent
  // blocks; last block keeps its last key — kShortenSeparators mode)
  size_t nb = tj.handles.size();
  std::vector<std::string> seps(nb);
  bool sep_key_plus_seq = false;
  for (size_t b = 0; b < nb; b++) {
    std::string sep(tj.last_keys[b].b, tj.last_keys[b].len);
    if (b + 1 < nb) {
      const BKey& nf = tj.first_keys[b + 1];
      shorten_separator(sep, (const uint8_t*)nf.b, nf.len);
      size_t su = sep.size() - 8, nu = (size_t)nf.len - 8;
      if (su == nu && memcmp(sep.data(), nf.b, su) == 0)
        sep_key_plus_seq = true;
    }
    seps[b] = sep;
  }
  TailStats st;
  st.num_data_blocks = nb;
  st.data_size = tj.image.len;
  st.num_entries = tj.file_count;
  for (uint64_t i = tj.file_first; i < tj.file_first + tj.file_count; i++) {
    st.raw_key_size += tj.klen[i];
    st.raw_value_size += tj.vlen[i];
  }
  st.num_deletions = tj.n_tomb;
  std::string tail = build_tail(tj.o, st, tj.handles, seps, !sep_key_plus_seq,
                                tj.image.len, tj.filter_content, tj.n_filter);
  tj.image.append(tail.data(), tail.size());
  // parallel segmented write: the last file's write sits on the job's
  // critical path
  if (!write_file_segmented(tj.path.c_str(), tj.image.p, tj.image.len,
                            16u << 20, 4))
    return -1;
  dcw_output_file of;
  memset(&of, 0, sizeof(of));
  snprintf(of.path, sizeof(of.path), "%s", tj.path.c_str());
  of.file_number = tj.o.orig_file_number;
  of.file_size = tj.image.len;
  const BKey& smallest = tj.first_keys.front();
  const BKey& largest = tj.last_keys.back();
  of.smallest_len = smallest.len;
  memcpy(of.smallest_ikey, smallest.b, smallest.len);
  of.largest_len = largest.len;
  memcpy(of.largest_ikey, largest.b, largest.len);
  of.smallest_seqno = tj.mn_seq == ~0ull ? 0 : tj.mn_seq;
  of.largest_seqno = tj.mx_seq;
  of.num_entries = tj.file_count;
  {
    std::lock_guard<std::mutex> lk(g_out_mu);
    tj.out->files[tj.slot] = of;
    tj.out->total_bytes += of.file_size;
  }
  return 0;
}

// GPU block plan: per-survivor next-block-start chain (k_plan_next)
struct PlanChain {
  const uint32_t* next = nullptr;
  const uint32_t* unc = nullptr;
  const uint16_t* nr = nullptr;
};
// Follow the chain from survivor `from` until the blocks cover min_unc
// bytes of output (identical FSM to plan_blocks).
std::vector<PlannedBlock> walk_plan_chain(const PlanChain& pc, size_t from,
                                          size_t nsurv, uint64_t min_unc) {
  std::vector<PlannedBlock> blocks;
  uint64_t produced = 0;
  size_t i = from;
  while (i < nsurv && produced < min_unc) {
    uint32_t nx = pc.next[i];
    PlannedBlock pb;
    pb.first = (uint32_t)i;
    pb.count = nx - (uint32_t)i;
    pb.unc_size = pc.unc[i];
    pb.num_restarts = pc.nr[i];
    blocks.push_back(pb);
    produced += pb.unc_size + kTrailerSize;
    i = nx;
  }
  return blocks;
}

// DCW_PARANOID: re-verify the trailers of the blocks just packed at `base`
void paranoid_verify(TailJob& f, const std::vector<PlannedBlock>& blocks,
                     const std::vector<uint32_t>& csizes,
                     const std::vector<uint64_t>& outoff, uint64_t base) {
  size_t take = outoff.size();
  for (void* e : f.pend) GpuJob::wait_event(e);
  for (size_t b = 0; b < take; b++) {
    const uint8_t* body = f.image.p + base + outoff[b];
    uint32_t stored;
    memcpy(&stored, body + csizes[b] + 1, 4);
    uint8_t ty = body[csizes[b]];
    uint32_t actual =
        block_checksum(f.o.checksum_type, &g_crc, body, csizes[b], ty);
    if (stored != actual) {
      fprintf(stderr,
              "[paranoid] chunk@%zu block %zu/%zu first=%u count=%u "
              "csize=%u type=%u stored=%08x actual=%08x\n",
              (size_t)f.file_first, b, take, blocks[b].first, blocks[b].count,
              csizes[b], ty, stored, actual);
      if (b > 2) break;
    }
  }
}

// handles, boundary keys and seq stats of the blocks just packed at `base`,
// from the kBlkStatStride records that emit_blocks prefetched
void collect_block_stats(TailJob& f, const uint8_t* stats,
                         const std::vector<uint32_t>& csizes,
                         const std::vector<uint64_t>& outoff, uint64_t base) {
  for (size_t b = 0; b < outoff.size(); b++) {
    f.handles.push_back({base + outoff[b], csizes[b]});
    const uint8_t* r = stats + b * GpuJob::kBlkStatStride;
    BKey fk, lk;
    fk.len = r[0];
    memcpy(fk.b, r + 1, fk.len);
    lk.len = r[64];
    memcpy(lk.b, r + 65, lk.len);
    f.first_keys.push_back(fk);
    f.last_keys.push_back(lk);
    uint64_t bmn, bmx, bt;
    memcpy(&bmn, r + 128, 8);
    memcpy(&bmx, r + 136, 8);
    memcpy(&bt, r + 144, 8);
    f.add_seq(bmn, bmx, bt);
  }
}

// partial block after a cut (1 entry for pure size cuts; up to a full
// block's worth for grandparent-rule cuts): gathered and built on the host
int emit_partial_block(GpuJob& job, TailJob& f, uint64_t first, uint32_t count,
                       std::string* err) {
  std::vector<std::pair<std::string, std::string>> kvs;
  if (job.gather_entries(first, count, &kvs, err) != 0) return -1;
  BlockBuilder bb(f.o.block_restart_interval, false);
  std::string lastk;
  for (auto& kv : kvs) {
    bb.AddWithLastKey((const uint8_t*)kv.first.data(), kv.first.size(),
                      (const uint8_t*)kv.second.data(), kv.second.size(),
                      (const uint8_t*)lastk.data(), lastk.size());
    lastk = kv.first;
  }
  std::string contents = bb.Finish();
  std::string pblk;
  SstIndexEntry h = append_block(pblk, f.o, (const uint8_t*)contents.data(),
                                 contents.size(), true);
  h.off += f.image.len;
  f.settle_before_growth(f.image.len + pblk.size());
  f.image.append(pblk.data(), pblk.size());
  f.handles.push_back(h);
  BKey fk, lk;
  fk.len = (uint8_t)kvs.front().first.size();
  memcpy(fk.b, kvs.front().first.data(), fk.len);
  lk.len = (uint8_t)kvs.back().first.size();
  memcpy(lk.b, kvs.back().first.data(), lk.len);
  f.first_keys.push_back(fk);
  f.last_keys.push_back(lk);
  for (auto& kv : kvs) {
    uint64_t tag;
    memcpy(&tag, kv.first.data() + kv.first.size() - 8, 8);
    uint8_t vt = (uint8_t)tag;
    // kTypeDeletion / kTypeSingleDeletion
    f.add_seq(tag >> 8, tag >> 8, vt == 0 || vt == 7);
  }
  return 0;
}

// what bbt_finish keeps across the files of one job
struct BbtRun {
  PlanChain plan;
  FileCutter cutter;
  double comp_ratio = 0.62; // adaptive: refined from the first chunk
  uint64_t plan_usec = 0, write_usec = 0;
};

// The data blocks of the file that starts at survivor f.file_first, chunk
// by chunk: plan -> GPU emit -> cut walk on csizes -> fetch only what the
// file keeps.  Sets f.file_count; the next file starts after it.
int build_bbt_data(JobCtx& c, BbtRun& run, TailJob& f) {
  const dcw_job_desc* d = c.d;
  GpuJob& job = c.job;
  const size_t nsurv = job.num_survivors();
  const size_t s = f.file_first;
  std::string err;
  size_t cur = s;
  FileCut fc;
  while (!fc.cut && cur < nsurv) {
    uint64_t tp0 = now_usec();
    uint64_t already = f.image.len;
    uint64_t want = d->target_file_size > already
                        ? d->target_file_size - already
                        : (64 << 10);
    uint64_t min_unc = f.o.compression == 1
                           ? (uint64_t)(want / run.comp_ratio) +
                                 (uint64_t)(want / run.comp_ratio) / 32 +
                                 16 * f.o.block_size
                           : want + 2 * f.o.block_size;
    std::vector<PlannedBlock> blocks =
        walk_plan_chain(run.plan, cur, nsurv, min_unc);
    run.plan_usec += now_usec() - tp0;
    c.wp.mark(kWpChainWalk);
    if (blocks.empty()) break;
    if (peek_cancel(d->job_id)) {
      consume_cancel(d->job_id);
      return fail(c.res, 30 /*DCW_CANCELLED*/, "job cancelled");
    }
    std::vector<uint32_t> csizes;
    c.wp.mark(kWpOther);
    if (job.emit_blocks(blocks, f.o, &csizes, &err) != 0)
      return fail(c.res, 21, err);
    c.wp.mark(kWpEmit);
    {
      uint64_t unc_sum = 0, c_sum = 0;
      for (auto& pb : blocks) unc_sum += pb.unc_size;
      for (auto cz : csizes) c_sum += cz;
      if (f.o.compression == 1 && unc_sum > 0)
        run.comp_ratio = 0.5 * run.comp_ratio + 0.5 * ((double)c_sum / unc_sum);
    }
    uint64_t old = f.image.len;
    fc = run.cutter.next_chunk(blocks, csizes, old, s, nsurv);
    // pack the fc.take full blocks that the file keeps behind its image
    std::vector<uint64_t> outoff(fc.take);
    uint64_t acc = 0;
    for (size_t b = 0; b < fc.take; b++) {
      outoff[b] = acc;
      acc += csizes[b] + kTrailerSize;
    }
    f.settle_before_growth(old + acc);
    f.image.resize_uninit(old + acc);
    void* ev = nullptr;
    if (job.pack_into(0, fc.take, outoff, f.image.p + old, acc, &ev, &err) != 0)
      return fail(c.res, 22, err);
    if (ev) f.pend.push_back(ev);
    if (getenv("DCW_PARANOID")) paranoid_verify(f, blocks, csizes, outoff, old);
    const uint8_t* stats = job.chunk_stats();
    if (!stats) return fail(c.res, 23, "no prefetched chunk stats");
    collect_block_stats(f, stats, csizes, outoff, old);
    c.wp.mark(kWpWalkPack);
    if (fc.take) cur = blocks[fc.take - 1].first + blocks[fc.take - 1].count;
    if (fc.take < blocks.size()) break; // cut decided inside this chunk
  }
  c.wp.mark(kWpOther);
  if (fc.cut && fc.partial_count > 0 &&
      emit_partial_block(job, f, fc.partial_first, fc.partial_count, &err) != 0)
    return fail(c.res, 24, err);
  c.wp.mark(kWpGather);
  if (fc.cut) cur = fc.cut_entry;
  f.file_count = cur - s;
  return 0;
}

int bbt_finish(JobCtx& c) {
  const dcw_job_desc* d = c.d;
  GpuJob& job = c.job;
  std::string err;
  const size_t nsurv = job.num_survivors();
  TableOpts base = opts_from_desc(d);

  PlanChain plan;
  if (nsurv > 0 &&
      job.plan_all(base, &plan.next, &plan.unc, &plan.nr, &err) != 0)
    return fail(c.res, 28, err);
  c.wp.mark(kWpPlan);

  // grandparent-aware file cutting: per-survivor boundary positions from
  // the GPU, the walk itself in FileCutter
  std::vector<uint32_t> gp_pos;
  std::vector<uint8_t> gp_nback;
  std::vector<uint64_t> gp_sizes;
  if (d->num_grandparents > 0) {
    if (job.gp_positions(d, &gp_pos, &gp_nback, &err) != 0)
      return fail(c.res, 27, err);
    for (uint32_t g = 0; g < d->num_grandparents; g++)
      gp_sizes.push_back(d->grandparents[g].file_size);
  }
  BbtRun run{plan,
             FileCutter(d->target_file_size, d->max_compaction_bytes,
                        d->level_compaction_dynamic_file_size != 0,
                        d->num_grandparents, gp_pos.data(), gp_nback.data(),
                        gp_sizes.data())};

  uint64_t next_file_number = d->next_file_number;
  BbtOutputs out;
  out.files.reserve(1024); // slots are written by tail threads; no realloc
  std::vector<std::future<int>> writers;
  // join tail threads on EVERY exit path (they write into out.files and
  // this stack frame's vectors; early error returns must not outlive them)
  struct WriterJoin {
    std::vector<std::future<int>>* w;
    ~WriterJoin() {
      for (auto& f : *w)
        if (f.valid()) (void)f.get();
    }
  } wj{&writers};
  uint64_t total_out_entries = 0;

  size_t s = 0;
  while (s < nsurv) {
    auto tj = std::make_shared<TailJob>();
    tj->o = base;
    tj->o.orig_file_number = next_file_number++;
    tj->image.reserve(d->target_file_size + (d->target_file_size >> 2) + (2u << 20));
    tj->file_first = s;
    tj->klen = job.plan_klen().data();
    tj->vlen = job.plan_vlen().data();
    tj->out = &out;
    if (int rc = build_bbt_data(c, run, *tj)) return rc;
    if (tj->handles.empty()) break; // nothing left
    // per-file bloom filter (built on the GPU from the file's survivors)
    if (tj->o.bloom_millibits_per_key && tj->file_count > 0) {
      if (job.filter_build(tj->file_first, tj->file_count,
                           tj->o.bloom_millibits_per_key, &tj->filter_content,
                           &tj->n_filter, &err) != 0)
        return fail(c.res, 37, err);
    }
    uint64_t tw1 = now_usec();
    // hand the whole per-file tail (separators, stats, meta tail, file
    // write) to a background thread — the GPU starts the next file now.
    tj->path = output_path(d, tj->o.orig_file_number);
    if (out.files.size() + 1 >= out.files.capacity()) {
      // join tail threads before the vector reallocates (slots are written
      // by threads through indices into this vector)
      for (auto& w : writers)
        if (w.get() != 0) return fail(c.res, 26, "output file tail/write failed");
      writers.clear();
      out.files.reserve(out.files.capacity() * 2);
    }
    tj->slot = out.files.size();
    out.files.emplace_back();
    total_out_entries += tj->file_count;
    s += tj->file_count;
    writers.emplace_back(
        tails().submit([tj]() -> int { return finish_bbt_file(*tj); }));
    run.write_usec += now_usec() - tw1;
    c.wp.mark(kWpTailSpawn);
  }
  {
    uint64_t tj2 = now_usec();
    c.wp.mark(kWpOther);
    for (auto& w : writers)
      if (w.get() != 0) return fail(c.res, 26, "output file tail/write failed");
    run.write_usec += now_usec() - tj2;
    c.wp.mark(kWpJoin);
  }
  job.drain_d2h();
  if (getenv("DCW_PHASE_DEBUG")) {
    const LoadedInputs& L = c.L;
    fprintf(stderr, "[phase]");
    for (int i = 0; i < kWpSlots; i++)
      fprintf(stderr, " %s=%.1fms", c.wp.names[i], c.wp.us[i] / 1000.0);
    fprintf(stderr, " total=%.1fms\n", (now_usec() - c.t_start) / 1000.0);
    fprintf(stderr,
            "[load] reset=%.1fms reserve=%.1fms pread=%.1fms stage=%.1fms "
            "parse=%.1fms (dzt_keycsum=%.1fms)\n",
            c.us_reset / 1000.0, L.us_reserve / 1000.0, L.us_pread / 1000.0,
            L.us_stage / 1000.0, L.us_parse / 1000.0,
            L.us_dzt_keycsum / 1000.0);
  }
  c.res->t_plan_usec = run.plan_usec;
  c.res->t_d2h_usec = (uint64_t)(job.ms_d2h * 1000);
  c.res->t_write_usec = run.write_usec;
  fill_result(c, out.files, out.total_bytes, total_out_entries);
  return 0;
}

// ---- DcwZipTable ("DZT1") output path: plan (dzt_plan_files) + build +
//      write; format: oracle/dzt.c ----
enum DztSlot {
  kDztSample, kDztValues, kDztKeyArea, kDztPack, kDztKIndex, kDztProps,
  kDztWrite, kDztMeta, kDztSlots
};
struct DztProf {
  const char* names[kDztSlots] = {"plan+dict", "values", "keyarea", "pack",
                                  "kindex",    "props",  "write",   "meta"};
  uint64_t us[kDztSlots] = {0};
  uint64_t t_last = 0;
  void mark(DztSlot slot) {
    uint64_t now = now_usec();
    us[slot] += now - t_last;
    t_last = now;
  }
};

void put32(std::string& s, uint32_t v) { s.append((const char*)&v, 4); }
void put64(std::string& s, uint64_t v) { s.append((const char*)&v, 8); }

// per-file dictionary (sampling rule identical to oracle/dzt.c)
int build_dzt_dict(GpuJob& job, const DztFilePlan& fp, std::string* dict,
                   std::string* err) {
  const auto& vlen = job.plan_vlen();
  std::vector<uint32_t> sidx;
  uint64_t stride = fp.count / 256;
  if (!stride) stride = 1;
  for (uint64_t j = 0; j < fp.count; j += stride)
    sidx.push_back((uint32_t)(fp.first + j));
  std::vector<uint8_t> samp(sidx.size() * 256);
  if (job.dzt_sample(sidx, samp.data(), err) != 0) return -1;
  for (size_t si = 0; si < sidx.size() && dict->size() < kDztDictMax; si++) {
    uint32_t take = vlen[sidx[si]] < kDztDictSampleBytes ? vlen[sidx[si]]
                                                         : kDztDictSampleBytes;
    if (dict->size() + take > kDztDictMax)
      take = (uint32_t)(kDztDictMax - dict->size());
    dict->append((const char*)samp.data() + si * 256, take);
  }
  return 0;
}

struct DztLayout { // section offsets in the file image
  uint64_t dict_off, value_off, kindex_off, vindex_off, props_off;
};

// props + footer (oracle/dzt.c layout); `image` holds [0, props_off)
std::string build_dzt_props_footer(const TableOpts& o, const DztFilePlan& fp,
                                   uint32_t U, const DztLayout& lay,
                                   const uint8_t* image,
                                   const std::string& dict,
                                   const std::string& kindex,
                                   const std::string& vindex) {
  std::string props;
  put64(props, fp.count);
  put64(props, fp.kbs.size());
  put64(props, fp.vbs.size());
  put64(props, dict.size());
  put64(props, fp.count * (uint64_t)(U + 8));
  put64(props, fp.raw_value);
  put64(props, o.orig_file_number);
  put64(props, o.creation_time);
  put64(props, o.file_creation_time);
  put32(props, U);
  put32(props, o.checksum_type);
  put32(props, o.cf_id);
  int32_t lvl = o.level_at_creation;
  props.append((const char*)&lvl, 4);
  for (const std::string* sp : {&o.db_id, &o.db_session_id, &o.db_host_id,
                                &o.cf_name}) {
    uint8_t tmp[10];
    int m = varint32_put(tmp, (uint32_t)sp->size());
    props.append((const char*)tmp, m);
    props.append(*sp);
  }
  uint32_t ct = o.checksum_type;
  auto csum = [ct](const void* p, size_t n) {
    return block_checksum(ct, &g_crc, (const uint8_t*)p, n, 0);
  };
  std::string footer;
  put64(footer, lay.dict_off);
  put64(footer, lay.value_off);
  put64(footer, lay.kindex_off);
  put64(footer, lay.vindex_off);
  put64(footer, lay.props_off);
  put64(footer, props.size());
  put32(footer, csum(image, lay.dict_off)); // key area
  put32(footer, csum(dict.data(), dict.size()));
  put32(footer, csum(kindex.data(), kindex.size()));
  put32(footer, csum(vindex.data(), vindex.size()));
  put32(footer, csum(props.data(), props.size()));
  put32(footer, ct);
  put32(footer, 1);  // version
  put32(footer, 0);  // pad
  put64(footer, 0);  // reserved
  put64(footer, 0x313050495A574344ull); // "DCWZIP01"
  return props + footer;
}

// Builds one DZT file image on the GPU and the host, starts its write in
// the background (dzt_writes) and fills the file's meta.
int build_dzt_file(JobCtx& c, const DztFilePlan& fp, const TableOpts& o,
                   uint32_t U, DztProf& prof,
                   std::vector<std::future<bool>>& dzt_writes,
                   dcw_output_file* of) {
  GpuJob& job = c.job;
  std::string err;
  const uint32_t IK = U + 8; // <= 56: fits the 64-byte ABI key fields
  std::vector<GpuJob::DztVBlock> vbs;
  std::vector<GpuJob::DztKBlock> kbs;
  for (auto& v : fp.vbs) vbs.push_back({v.first, v.count, v.ulen, v.stage_off});
  for (auto& k : fp.kbs) kbs.push_back({k.first, k.count, k.koff});
  std::string dict;
  if (build_dzt_dict(job, fp, &dict, &err) != 0) return fail(c.res, 31, err);
  prof.mark(kDztSample);
  // ---- value blocks on the GPU ----
  std::vector<uint32_t> csize, csum;
  std::vector<uint8_t> btype;
  if (job.dzt_values(vbs, fp.voff, fp.first, (const uint8_t*)dict.data(),
                     (uint32_t)dict.size(), o, &csize, &btype, &csum,
                     &err) != 0)
    return fail(c.res, 32, err);
  prof.mark(kDztValues);
  std::vector<uint64_t> outoff(vbs.size());
  uint64_t vtotal = 0;
  for (size_t b = 0; b < vbs.size(); b++) {
    outoff[b] = vtotal;
    vtotal += csize[b] + 5;
  }
  size_t nkb = kbs.size();
  DztLayout lay;
  lay.dict_off = fp.key_area_size;
  lay.value_off = lay.dict_off + dict.size();
  lay.kindex_off = lay.value_off + vtotal;
  lay.vindex_off = lay.kindex_off + (uint64_t)nkb * (IK + 20);
  lay.props_off = lay.vindex_off + (uint64_t)vbs.size() * 24;
  // ---- GPU emits straight into the host image ----
  RawBuf image;
  std::vector<uint8_t> first_ikeys((uint64_t)nkb * IK);
  image.reserve(lay.props_off + (64u << 10)); // props+footer appended after
  image.resize_uninit(lay.props_off);
  if (job.dzt_keyarea(kbs, fp.voff, fp.first, fp.key_area_size, U, image.p,
                      first_ikeys.data(), &err) != 0)
    return fail(c.res, 33, err);
  prof.mark(kDztKeyArea);
  memcpy(image.p + lay.dict_off, dict.data(), dict.size());
  if (job.dzt_pack_values(vbs, outoff, vtotal, image.p + lay.value_off,
                          &err) != 0)
    return fail(c.res, 34, err);
  prof.mark(kDztPack);
  std::string kindex;
  kindex.reserve(lay.vindex_off - lay.kindex_off);
  for (size_t kb = 0; kb < nkb; kb++) {
    kindex.append((const char*)first_ikeys.data() + kb * IK, IK);
    put64(kindex, kbs[kb].koff);
    uint64_t kend = kb + 1 < nkb ? kbs[kb + 1].koff : fp.key_area_size;
    put32(kindex, (uint32_t)(kend - kbs[kb].koff));
    put64(kindex, kbs[kb].first - fp.first);
  }
  prof.mark(kDztKIndex);
  memcpy(image.p + lay.kindex_off, kindex.data(), kindex.size());
  std::string vindex;
  vindex.reserve(lay.props_off - lay.vindex_off);
  for (size_t b = 0; b < vbs.size(); b++) {
    put64(vindex, outoff[b]);
    put32(vindex, csize[b]);
    put32(vindex, vbs[b].ulen);
    put64(vindex, vbs[b].first - fp.first);
  }
  memcpy(image.p + lay.vindex_off, vindex.data(), vindex.size());
  std::string pf =
      build_dzt_props_footer(o, fp, U, lay, image.p, dict, kindex, vindex);
  image.append(pf.data(), pf.size());
  prof.mark(kDztProps);
  // ---- write + meta ----
  std::string path = output_path(c.d, o.orig_file_number);
  // segmented parallel write on a background task, overlapping the next
  // file's GPU phases (the write was the dominant configs[3] cost)
  const uint64_t image_len = image.len; // meta reads it after the swap
  {
    // bound in-flight images: each holds a pinned buffer; unbounded
    // overlap forces fresh hipHostMalloc pins that cost more than the
    // write overlap saves
    while (dzt_writes.size() >= 2) {
      if (!dzt_writes.front().get())
        return fail(c.res, 35, "DZT output file write failed");
      dzt_writes.erase(dzt_writes.begin());
    }
    auto img = std::make_shared<RawBuf>();
    image.swap(*img);
    dzt_writes.emplace_back(std::async(std::launch::async, [img, path]() {
      return write_file_segmented(path.c_str(), img->p, img->len, 32u << 20, 8);
    }));
  }
  prof.mark(kDztWrite);
  memset(of, 0, sizeof(*of));
  snprintf(of->path, sizeof(of->path), "%s", path.c_str());
  of->file_number = o.orig_file_number;
  of->file_size = image_len;
  memcpy(of->smallest_ikey, first_ikeys.data(), IK);
  of->smallest_len = IK;
  std::vector<std::pair<std::string, std::string>> lastkv;
  if (job.gather_entries(fp.first + fp.count - 1, 1, &lastkv, &err) != 0)
    return fail(c.res, 36, err);
  memcpy(of->largest_ikey, lastkv[0].first.data(), IK);
  of->largest_len = IK;
  uint64_t mn, mx, tomb;
  if (job.seq_minmax(fp.first, fp.count, &mn, &mx, &tomb, &err) != 0)
    return fail(c.res, 36, err);
  of->smallest_seqno = mn == ~0ull ? 0 : mn;
  of->largest_seqno = mx;
  of->num_entries = fp.count;
  prof.mark(kDztMeta);
  return 0;
}

// DcwZipTable output (BASELINE configs[3]): same decode/merge/dedup
// pipeline, different build path
int dzt_finish(JobCtx& c) {
  const dcw_job_desc* d = c.d;
  GpuJob& job = c.job;
  // The format has one user-key length U per file and the oracle's builder
  // takes it from the survivors (orc_dzt_builder_add), not from the inputs.
  // Fast mode: the job's uniform length.  General-key mode: the survivors'
  // lengths (plan metadata) must all be equal — any U in 1..48 then.
  uint32_t U = job.ukey_len;
  if (job.general_keys) {
    const std::vector<uint8_t>& klen = job.plan_klen();
    for (size_t i = 1; i < job.num_survivors(); i++)
      if (klen[i] != klen[0])
        return fail(c.res, 29, "DcwZipTable requires uniform user-key length");
    if (job.num_survivors()) U = (uint32_t)klen[0] - 8;
    // the decoders refuse empty user keys (klen < 9) before this; should one
    // ever get here, refuse it as an envelope matter, not in the key emit
    if (job.num_survivors() && U == 0)
      return fail(c.res, 29, "DcwZipTable requires a user-key length of "
                             "1..48 (outside envelope)");
  }
  std::vector<DztFilePlan> files =
      dzt_plan_files(job.plan_vlen().data(), job.plan_shared().data(),
                     job.num_survivors(), U, d->target_file_size);
  TableOpts o = opts_from_desc(d);
  uint64_t next_file_number = d->next_file_number;
  std::vector<dcw_output_file> out_files;
  uint64_t total_out_bytes = 0, total_out_entries = 0;
  std::vector<std::future<bool>> dzt_writes; // per-file background writes
  DztProf prof;
  for (auto& fp : files) {
    prof.t_last = now_usec();
    o.orig_file_number = next_file_number++;
    dcw_output_file of;
    if (int rc = build_dzt_file(c, fp, o, U, prof, dzt_writes, &of)) return rc;
    out_files.push_back(of);
    total_out_bytes += of.file_size;
    total_out_entries += fp.count;
  }
  for (auto& w : dzt_writes)
    if (!w.get()) return fail(c.res, 35, "DZT output file write failed");
  if (getenv("DCW_PHASE_DEBUG")) {
    fprintf(stderr, "[dzt]");
    for (int i = 0; i < kDztSlots; i++)
      fprintf(stderr, " %s=%.1fms", prof.names[i], prof.us[i] / 1000.0);
    fprintf(stderr, "\n");
  }
  fill_result(c, out_files, total_out_bytes, total_out_entries);
  if (getenv("DCW_PHASE_DEBUG"))
    fprintf(stderr,
            "[phase] dzt total=%.1fms ms_decode=%.2f ms_merge=%.2f "
            "ms_dedup=%.2f\n"
            "[load] pread=%.1fms stage=%.1fms parse=%.1fms "
            "(dzt_keycsum=%.1fms)\n",
            (now_usec() - c.t_start) / 1000.0, job.ms_decode, job.ms_merge,
            job.ms_dedup, c.L.us_pread / 1000.0, c.L.us_stage / 1000.0,
            c.L.us_parse / 1000.0, c.L.us_dzt_keycsum / 1000.0);
  return 0;
}

} // namespace
} // namespace dcw

using namespace dcw;

extern "C" {

const char* dcw_version(void) { return "toplingdb_amd dcompact worker r2 (gfx950)"; }

static void dcw_segv_handler(int sig, siginfo_t* si, void*) {
  char buf[128];
  int m = snprintf(buf, sizeof(buf), "[segv] sig=%d fault_addr=%p\n", sig,
                   si ? si->si_addr : nullptr);
  ssize_t w = write(2, buf, m);
  (void)w;
  void* frames[64];
  int n = backtrace(frames, 64);
  backtrace_symbols_fd(frames, n, 2);
  _exit(139);
}

int32_t dcw_init(int32_t device_ordinal) {
  if (getenv("DCW_SEGV_TRACE")) {
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_sigaction = dcw_segv_handler;
    sa.sa_flags = SA_SIGINFO;
    sigaction(SIGSEGV, &sa, nullptr);
    sigaction(SIGBUS, &sa, nullptr);
    sigaction(SIGABRT, &sa, nullptr);
  }
  std::lock_guard<std::mutex> lk(g_mu);
  std::string err;
  if (gpu_init(device_ordinal, &err) != 0) {
    fprintf(stderr, "dcw_init: %s\n", err.c_str());
    return -1;
  }
  g_inited = true;
  return 0;
}

void dcw_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto& kv : g_staged) delete kv.second;
  g_staged.clear();
  g_pin_pool.drain();
  gpu_shutdown();
  g_inited = false;
}

void dcw_cancel(int32_t job_id) {
  std::lock_guard<std::mutex> lk(g_cancel_mu);
  g_cancelled.insert(job_id);
}

void dcw_free_result(dcw_job_result* res) {
  free(res->files);
  res->files = nullptr;
  res->num_files = 0;
}

uint64_t dcw_stage_inputs(const dcw_job_desc* d) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_inited) return 0;
  std::string err;
  LoadedInputs L;
  if (load_inputs(d, &L, &err) != 0) {
    fprintf(stderr, "dcw_stage_inputs: %s\n", err.c_str());
    return 0;
  }
  GpuJob job;
  if (job.stage(L.gi, &err) != 0) {
    fprintf(stderr, "dcw_stage_inputs: %s\n", err.c_str());
    return 0;
  }
  StagedJob* sj = new StagedJob;
  if (job.stage_release(&sj->dev, &err) != 0) {
    delete sj;
    return 0;
  }
  sj->in_bytes = L.in_bytes;
  sj->tombstones = std::move(L.tombstones);
  uint64_t h = g_next_stage_handle++;
  g_staged[h] = sj;
  return h;
}

void dcw_release_staged(uint64_t handle) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_staged.find(handle);
  if (it != g_staged.end()) {
    delete it->second;
    g_staged.erase(it);
  }
}

int32_t dcw_execute(const dcw_job_desc* d, dcw_job_result* res) {
  memset(res, 0, sizeof(*res));
  if (int rc = check_desc(d, res)) return rc;

  uint64_t t_start = now_usec();
  struct PooledJob {
    GpuJob* j;
    PooledJob() : j(g_jobs.acquire()) {}
    ~PooledJob() { g_jobs.put(j); }
  } pj;
  pj.j->reset();
  JobCtx c{d, res, *pj.j, t_start};
  c.wp.t_last = t_start;
  c.us_reset = now_usec() - t_start;

  if (int rc = acquire_inputs(c)) return rc;
  res->t_read_usec = now_usec() - t_start;
  if (int rc = run_front(c)) return rc;
  return d->output_table_factory == 1 ? dzt_finish(c) : bbt_finish(c);
}

int32_t dcw_gen_sst(const char* path, uint64_t seed, uint64_t num_entries,
                    uint32_t key_len, uint32_t value_len, uint64_t seq_base,
                    uint32_t compression, uint32_t checksum_type,
                    uint64_t file_number, const char* db_id,
                    const char* db_session_id, uint64_t current_time) {
  if (checksum_type != 0 && checksum_type != 1 && checksum_type != 4) return -1;
  TableOpts o;
  o.compression = compression;
  o.checksum_type = checksum_type;
  o.db_id = db_id ? db_id : "";
  o.db_session_id = db_session_id ? db_session_id : "";
  o.db_host_id = "dcw-host";
  o.orig_file_number = file_number;
  o.creation_time = current_time;
  o.file_creation_time = current_time;
  return gen_sst_file(path, seed, num_entries, key_len, value_len, seq_base, o);
}

} // extern "C"
