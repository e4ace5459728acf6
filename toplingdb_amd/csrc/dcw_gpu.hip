// dcw_gpu.hip — MI355X (gfx950) device pipeline of the dcompact worker: the
// one GPU translation unit.  This file is the host runtime of GpuJob
// (staging, phase drivers, buffer owners, phase timing, kernel statistics);
// the kernels are included below from the dcw_k_*.h headers.
//
// GPU counterparts of the reference CPU hot loops:
//  - dcw_k_decode.h: k_verify_usize / k_decompress / k_count_entries /
//    k_decode_entries:
//      BlockFetcher::ReadBlockContents + DataBlockIter::ParseNextDataKey
//      (table/block_fetcher.cc:242, table/block_based/block.cc:37-139,667) —
//      restart-interval-parallel decode of prefix-compressed blocks.
//  - dcw_k_merge.h: k_merge_pair: the k-way merge (table/compaction_merging_iterator.cc)
//      recast as merge-path partitioned pairwise merges over 32-byte
//      normalized entries (ulong4), stable on ties (lower run first, like
//      the heap's child order).
//  - dcw_k_merge.h: k_mark_heads / k_group_fsm / gather: CompactionIterator::NextFromInput
//      + PrepareOutput (db/compaction/compaction_iterator.cc:475-1341) as a
//      per-user-key-group FSM.
//  - dcw_k_emit.h: k_emit / k_compress / k_checksum / k_pack: BlockBuilder +
//      BlockBasedTableBuilder write path (block_builder.cc:189-253,
//      block_based_table_builder.cc:1277-1330) — block-parallel encode,
//      DCW-deterministic snappy, XXH3/CRC32C trailers.
//
// Design notes (MI355X): integer/byte, HBM-bound work — no MFMA.  Loads are
// vectorized where layout permits (ulong4 = 32 B/entry merge moves); the
// snappy encoder keeps its 16 KiB hash table in LDS; launches are
// grid-strided and sized ≫256 workgroups to fill 8 XCDs.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <sys/time.h>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

#include "dcw_gpu.h"

// the kernels, in pipeline order (one translation unit)
#include "dcw_k_decode.h"
#include "dcw_k_merge.h"
#include "dcw_k_emit.h"
#include "dcw_k_filter_dzt.h"
#include "dcw_k_dzt_in.h"

namespace dcw {

// ------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------
#define HIPCHK(x)                                                      \
  do {                                                                 \
    hipError_t _e = (x);                                               \
    if (_e != hipSuccess) {                                            \
      if (err) *err = std::string("HIP error: ") + hipGetErrorString(_e) + \
                      " at " #x;                                       \
      return -1;                                                       \
    }                                                                  \
  } while (0)

static int g_device = -1;

int gpu_init(int ordinal, std::string* err) {
  hipError_t e = hipSetDevice(ordinal);
  if (e != hipSuccess) {
    if (err) *err = std::string("hipSetDevice: ") + hipGetErrorString(e);
    return -1;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= ordinal) {
    if (err) *err = "no HIP device";
    return -1;
  }
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, ordinal);
  if (e != hipSuccess) {
    if (err) *err = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
    return -1;
  }
  g_device = ordinal;
  return 0;
}
void gpu_shutdown() { g_device = -1; }
bool gpu_available() { return g_device >= 0; }

// ------------------------------------------------------------------
// owners: device buffers, pinned host buffers, events
// ------------------------------------------------------------------
// Grow-only device buffer.  Every device allocation a GpuJob owns is one of
// these, so the job's destructor frees them all without naming any.
// reserve() keeps the allocation when it is large enough and otherwise
// replaces it (contents are NOT preserved) with need + 25% + 64 B; kernels
// rely on that >= 64 B of slack past `need` (ByteWin::fill).
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
    return *this;
  }
  ~DevBuf() {
    if (p_) (void)hipFree(p_);
  }
  hipError_t reserve(size_t need) {
    if (p_ && cap_ >= need) return hipSuccess;
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
    size_t c = need + need / 4 + 64;
    hipError_t e = hipMalloc((void**)&p_, c);
    if (e == hipSuccess) cap_ = c;
    return e;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  // give up ownership (stage_release hands the staged input to a StagedInput)
  T* release() {
    T* r = p_;
    p_ = nullptr;
    cap_ = 0;
    return r;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0; // bytes
};

// Grow-only pinned host buffer, same growth policy.  With allow_pageable a
// failed pin falls back to malloc (slower copies, still correct).
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept
      : p_(o.p_), cap_(o.cap_), pageable_(o.pageable_) {
    o.p_ = nullptr;
    o.cap_ = 0;
  }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
    std::swap(pageable_, o.pageable_);
    return *this;
  }
  ~PinnedBuf() { drop(); }
  hipError_t reserve(size_t need, bool allow_pageable = false) {
    if (p_ && cap_ >= need) return hipSuccess;
    drop();
    size_t c = need + need / 4 + 64;
    hipError_t e = hipHostMalloc(&p_, c, hipHostMallocDefault);
    pageable_ = false;
    if (e != hipSuccess && allow_pageable) {
      p_ = malloc(c);
      pageable_ = true;
      e = p_ ? hipSuccess : hipErrorOutOfMemory;
    }
    if (e != hipSuccess) p_ = nullptr;
    cap_ = p_ ? c : 0;
    return e;
  }
  void* get() const { return p_; }
  size_t cap() const { return cap_; }

 private:
  void drop() {
    if (p_ && pageable_) free(p_);
    else if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  void* p_ = nullptr;
  size_t cap_ = 0;
  bool pageable_ = false;
};

// owning HIP event
struct Event {
  hipEvent_t e = nullptr;
  Event() { (void)hipEventCreate(&e); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { (void)hipEventDestroy(e); }
  operator hipEvent_t() const { return e; }
};

static double ms_between(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  (void)hipEventElapsedTime(&ms, a, b);
  return (double)ms;
}

// Times one phase on the job stream: records the start on construction,
// stop() records the end, and add() — after the stream sync the phase does
// anyway — accumulates the elapsed time.  Both events die with the scope,
// whichever way the phase returns.
class PhaseTimer {
 public:
  PhaseTimer(hipStream_t s, double* accum) : s_(s), accum_(accum) {
    (void)hipEventRecord(t0_, s_);
  }
  void stop() { (void)hipEventRecord(t1_, s_); }
  // `from` replaces the start event (split staging started the clock earlier)
  void add(hipEvent_t from = nullptr) { *accum_ += ms_between(from ? from : t0_, t1_); }

 private:
  hipStream_t s_;
  double* accum_;
  Event t0_, t1_;
};

// ------------------------------------------------------------------
// per-kernel timing (HIP events on the pipeline stream) + algorithmic
// byte accounting, for bench.py's roofline object
// ------------------------------------------------------------------
struct KStat {
  uint64_t launches = 0;
  double ms = 0;
  double alg_bytes = 0;
};
static std::map<std::string, KStat>& kstats() {
  static std::map<std::string, KStat> m;
  return m;
}
static std::mutex g_kmu;

struct KEv {
  const char* name;
  double bytes;
  hipEvent_t a, b;
};

struct GpuJob::Impl {
  hipStream_t stream = nullptr;
  hipStream_t d2h_stream = nullptr;
  // double-buffered pack->D2H: out_img slots with completion events so the
  // next file's emit kernels overlap the previous file's output transfer
  struct OutSlot {
    DevBuf<uint8_t> img;
    Event t0; // D2H start (on d2h_stream)
    Event done;
    bool pending = false;
  } outslots[2];
  int cur_outslot = 0;
  PinnedBuf h_keys; // pinned block-stats records (BLKSTAT_STRIDE each)
  // Pinned metadata arena: every small H2D copy stages through a linear
  // pinned allocation that is never reused within a job, then
  // hipMemcpyAsync on this job's own stream.  Keeps every copy ordered
  // within the job without NULL-stream synchronization (which would
  // serialize independent jobs sharing the device) and without per-copy
  // events.  arena_reset() is called from reset() when the stream
  // is idle (job boundaries), so in-flight copies never see reuse.
  std::vector<PinnedBuf> meta_blocks;
  size_t meta_cur_block = 0;
  size_t meta_off = 0;

  void arena_reset() {
    // grow-only: a job stages ~20-40 MB of metadata through 10-30 blocks,
    // and the old keep-one-block policy re-freed and re-pinned them every
    // job — hipHostFree is device-synchronizing and the cycle cost
    // ~200 ms/job of pipeline wall.  Keep everything up to a cap and only
    // trim (smallest first) beyond it.
    const size_t kArenaCap = 512u << 20;
    size_t total = 0;
    for (auto& b : meta_blocks) total += b.cap();
    static const bool dbg = getenv("DCW_PHASE_DEBUG") != nullptr;
    if (dbg)
      fprintf(stderr, "[arena] blocks=%zu total=%.1fMB\n", meta_blocks.size(),
              total / 1048576.0);
    while (total > kArenaCap && meta_blocks.size() > 1) {
      size_t small = 0;
      for (size_t i = 1; i < meta_blocks.size(); i++)
        if (meta_blocks[i].cap() < meta_blocks[small].cap()) small = i;
      total -= meta_blocks[small].cap();
      meta_blocks.erase(meta_blocks.begin() + small);
    }
    meta_cur_block = 0;
    meta_off = 0;
  }
  hipError_t h2d_meta(void* dst, const void* src, size_t n) {
    if (n == 0) return hipSuccess;
    static const bool sync_meta = getenv("DCW_SYNC_META") != nullptr;
    if (sync_meta) {
      // a NULL-stream hipMemcpy does NOT order against these NON-BLOCKING
      // job streams (caught by the suite: a grandparent-cut SST differed
      // by one byte under this env) — stage on the job stream and drain
      hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice,
                                    stream);
      if (e != hipSuccess) return e;
      return hipStreamSynchronize(stream);
    }
    size_t need = (n + 63) & ~(size_t)63;
    while (meta_cur_block < meta_blocks.size() &&
           meta_off + need > meta_blocks[meta_cur_block].cap()) {
      meta_cur_block++;
      meta_off = 0;
    }
    if (meta_cur_block >= meta_blocks.size()) {
      PinnedBuf b;
      hipError_t e = b.reserve(need > (1u << 20) ? need : (1u << 20));
      if (e != hipSuccess) return e;
      meta_blocks.push_back(std::move(b));
      meta_off = 0;
    }
    uint8_t* stagep = (uint8_t*)meta_blocks[meta_cur_block].get() + meta_off;
    meta_off += need;
    memcpy(stagep, src, n);
    return hipMemcpyAsync(dst, stagep, n, hipMemcpyHostToDevice, stream);
  }
  std::vector<KEv> kpending;
  void kbegin(const char* n, double bytes) {
    KEv e{n, bytes, nullptr, nullptr};
    (void)hipEventCreate(&e.a);
    (void)hipEventCreate(&e.b);
    (void)hipEventRecord(e.a, stream);
    kpending.push_back(e);
  }
  void kend() { (void)hipEventRecord(kpending.back().b, stream); }
  void kresolve() { // call after a stream sync
    std::lock_guard<std::mutex> lk(g_kmu);
    for (auto& e : kpending) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, e.a, e.b);
      KStat& s = kstats()[e.name];
      s.launches++;
      s.ms += ms;
      s.alg_bytes += e.bytes;
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
    kpending.clear();
  }
  // staged input: d_blob/d_boff/d_bsize are ALIASES (never freed through
  // these names) of either this job's own slots or a StagedInput's buffers
  uint8_t* d_blob = nullptr;
  uint64_t* d_boff = nullptr;
  uint32_t* d_bsize = nullptr;
  DevBuf<uint8_t> d_blob_own;
  DevBuf<uint64_t> d_boff_own;
  DevBuf<uint32_t> d_bsize_own;
  uint32_t n_blocks = 0;
  uint32_t checksum_type = 4;
  // decode
  DevBuf<uint32_t> d_usize;
  DevBuf<uint8_t> d_btype_in;
  DevBuf<uint64_t> d_uoff;
  DevBuf<uint8_t> d_ublob;
  uint64_t ublob_size = 0;
  DevBuf<uint32_t> d_nrestarts, d_iv_block, d_iv_local, d_iv_cnt, d_iv_base;
  uint32_t n_intervals = 0;
  DevBuf<uint32_t> d_err; // device error word (DevErr), first error wins
  DevBuf<uint32_t> d_uklen_probe;
  DevBuf<Crc32cTables> d_crc;
  // entries
  DevBuf<ulong4> d_ent[2];
  DevBuf<uint64_t> d_voff;
  DevBuf<uint32_t> d_vlen;
  DevBuf<uint8_t> d_klen;
  uint64_t n_entries = 0;
  std::vector<uint64_t> run_entry_begin;
  int final_buf = 0;
  // dedup
  DevBuf<uint8_t> d_head;
  DevBuf<uint64_t> d_headidx;
  uint64_t n_groups = 0;
  DevBuf<uint8_t> d_survive;
  DevBuf<uint64_t> d_newtag;
  DevBuf<uint8_t> d_clearv, d_gflags;
  DevBuf<uint32_t> d_pos;
  DevBuf<uint64_t> d_snaps;
  // levels-below device copies
  DevBuf<uint64_t> d_lb_sm0, d_lb_sm1, d_lb_lg0, d_lb_lg1;
  DevBuf<uint32_t> d_lb_beg, d_lb_smlen, d_lb_lglen;
  DevBuf<uint8_t> d_lb_smext, d_lb_lgext; // general-key mode: boundary bytes
  // survivors
  DevBuf<uint64_t> d_sk0, d_sk1, d_stag, d_svoff;
  DevBuf<uint32_t> d_svlen;
  DevBuf<uint8_t> d_sklen, d_sshared;
  uint64_t n_surv = 0;
  // emit chunk state
  DevBuf<EmitBlockDesc> d_bds;
  DevBuf<uint8_t> d_ucblob, d_cblob;
  DevBuf<uint32_t> d_ebsize; // one allocation: bsize[nb] csum[nb] btype[nb]
  uint32_t* d_ecsum = nullptr; // views into d_ebsize, not owners
  uint8_t* d_ebtype = nullptr;
  DevBuf<uint32_t> d_bigidx; // blocks over SNAP_MAX_UNC (k_compress_large)
  uint32_t emit_nblocks = 0;
  uint64_t emit_base = 0; // survivor index offset of this chunk's eoff array
  // misc scratch
  DevBuf<uint32_t> d_scan_bs; // scan_u8 per-block sums
  DevBuf<uint64_t> d_outoff;  // shared by pack_into (BBT) and dzt_pack_values
  DevBuf<uint8_t> d_scratch_keys;
  DevBuf<uint64_t> d_scratch_recoff;
  DevBuf<uint8_t> d_scratch_gather;
  DevBuf<unsigned long long> d_scratch_mm;
  DevBuf<uint64_t> d_merge_diag;
  DevBuf<uint64_t> d_gp_sm0, d_gp_sm1, d_gp_lg0, d_gp_lg1;
  DevBuf<uint8_t> d_gp_tie, d_gp_nback;
  DevBuf<uint32_t> d_gp_pos, d_gp_smlen, d_gp_lglen;
  DevBuf<uint32_t> d_plan_next, d_plan_meta;
  DevBuf<uint16_t> d_plan_nr;
  // DZT output path
  DevBuf<uint32_t> d_dzt_idx, d_dzt_voff, d_dzt_dict_tab, d_dzt_bsize, d_dzt_csum;
  DevBuf<uint8_t> d_dzt_sample, d_dzt_vstage, d_dzt_dict, d_dzt_cblob,
      d_dzt_btype, d_dzt_keyarea, d_dzt_kidx, d_dzt_img;
  DevBuf<DztVBlock> d_dzt_vbs;
  DevBuf<DztKBlock> d_dzt_kbs;
  uint64_t dzt_ccap = 0;
  DevBuf<uint64_t> d_rd_k0, d_rd_k1, d_rd_seq;
  DevBuf<uint32_t> d_rd_len;
  DevBuf<uint8_t> d_rd_ext; // general-key mode: fragment start bytes
  bool staged_split = false; // stage_begin/chunk in progress
  Event stage_t0;            // recorded by stage_begin
  DevBuf<uint8_t> d_kext;    // general-key side table (48 B/entry full ukeys)
  DevBuf<uint32_t> d_sw;     // survivor -> original payload index
  DevBuf<uint64_t> d_flush_offs; // flush-offload record offsets
  // DZT input path: host-built tables (dcw_k_dzt_in.h) + per-block btype
  DevBuf<DztVbIn> d_dzi_vbs;
  DevBuf<DztKbIn> d_dzi_kbs;
  DevBuf<DztFileIn> d_dzi_files;
  DevBuf<uint8_t> d_dzi_btype;
  std::vector<DztVbIn> h_dzi_vbs;
  std::vector<DztKbIn> h_dzi_kbs; // out_base filled once entry counts are known
  uint64_t dzi_ulen_total = 0;    // decoded bytes of all DZT value blocks
  uint64_t dzi_ubase = 0;         // where they start in d_ublob
  DevBuf<uint64_t> d_fhash;      // per-file filter hashes
  DevBuf<uint32_t> d_filter;     // filter bit array
  PinnedBuf h_plan; // host landing for next+meta (pageable if pinning fails)

  ~Impl() { // a job that failed mid-phase left its kernel events pending
    for (auto& e : kpending) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
  }

  // per-job device constants: CRC tables uploaded, error word cleared,
  // user-key-length probe armed
  int arm_consts(std::string* err) {
    HIPCHK(d_crc.reserve(sizeof(Crc32cTables)));
    HIPCHK(hipMemcpyAsync(d_crc, &g_crc, sizeof(Crc32cTables),
                          hipMemcpyHostToDevice, stream));
    HIPCHK(d_err.reserve(8));
    HIPCHK(hipMemsetAsync(d_err, 0, 8, stream));
    HIPCHK(d_uklen_probe.reserve(4));
    HIPCHK(hipMemsetAsync(d_uklen_probe, 0xff, 4, stream));
    return 0;
  }

  // Fetch the device error word and drain the stream.  A phase that ends
  // here passes its timer: the end event is recorded behind the fetch and
  // the elapsed time added after the sync.  A set word fails the call with
  // "<what> failed, code <n>"; with what == nullptr the caller inspects
  // *code itself.
  int check_err(const char* what, std::string* err, uint32_t* code = nullptr,
                PhaseTimer* phase = nullptr) {
    uint32_t e = 0;
    if (code) *code = 0;
    HIPCHK(hipMemcpyAsync(&e, d_err, 4, hipMemcpyDeviceToHost, stream));
    if (phase) phase->stop();
    HIPCHK(hipStreamSynchronize(stream));
    if (phase) {
      phase->add();
      kresolve();
    }
    if (code) *code = e;
    if (e && what) {
      if (err) *err = std::string(what) + " failed, code " + std::to_string(e);
      return -1;
    }
    return 0;
  }
};

GpuJob::GpuJob() : p_(new Impl) {
  unsigned sf = getenv("DCW_BLOCKING_STREAMS") ? hipStreamDefault
                                                : hipStreamNonBlocking;
  (void)hipStreamCreateWithFlags(&p_->stream, sf);
  (void)hipStreamCreateWithFlags(&p_->d2h_stream, sf);
}

void GpuJob::wait_event(void* done_event) {
  if (done_event) (void)hipEventSynchronize((hipEvent_t)done_event);
}

void GpuJob::drain_d2h() {
  for (auto& s : p_->outslots) {
    if (!s.pending) continue;
    (void)hipEventSynchronize(s.done);
    ms_d2h += ms_between(s.t0, s.done);
    s.pending = false;
  }
}

// Reuse this job object for a new job: keep device buffers (grow-only),
// reset the per-job state.  Staged-input pointers are dropped (borrowed
// buffers belong to their StagedInput; owned ones are kept in their slots).
void GpuJob::reset() {
  Impl* p = p_;
  static const bool dbg = getenv("DCW_PHASE_DEBUG") != nullptr;
  auto us = [] {
    struct timeval tv;
    gettimeofday(&tv, nullptr);
    return (uint64_t)tv.tv_sec * 1000000 + tv.tv_usec;
  };
  uint64_t t0 = dbg ? us() : 0;
  (void)hipStreamSynchronize(p->stream);
  (void)hipStreamSynchronize(p->d2h_stream);
  uint64_t t1 = dbg ? us() : 0;
  p->arena_reset();
  if (dbg)
    fprintf(stderr, "[reset] sync=%.1fms arena=%.1fms\n", (t1 - t0) / 1000.0,
            (us() - t1) / 1000.0);
  // own-slot staged buffers are grow-only (kept for the next job);
  // borrowed ones belong to their StagedInput — either way just unalias
  p->d_blob = nullptr;
  p->d_boff = nullptr;
  p->d_bsize = nullptr;
  p->n_blocks = 0;
  p->n_entries = 0;
  p->n_surv = 0;
  p->run_entry_begin.clear();
  p->final_buf = 0;
  p->emit_nblocks = 0;
  p->emit_base = 0;
  n_entries_ = 0;
  n_surv_ = 0;
  ukey_len = 0;
  general_keys = false;
  h_shared_.clear();
  h_klen_.clear();
  h_vlen_.clear();
  run_blocks_.clear();
  dzt_files_.clear();
  rd_frags_.clear();
  ms_decode = ms_merge = ms_dedup = ms_emit = ms_h2d = ms_d2h = 0;
}
GpuJob::~GpuJob() {
  Impl* p = p_;
  // drain both streams; the buffers and events then go with the Impl
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->d2h_stream) (void)hipStreamSynchronize(p->d2h_stream);
  if (p->d2h_stream) (void)hipStreamDestroy(p->d2h_stream);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

static uint32_t grid_for(uint64_t work, uint32_t block = 256) {
  uint64_t g = (work + block - 1) / block;
  if (g > 4096) g = 4096; // grid-stride beyond (≫256 WGs fills 8 XCDs)
  if (g == 0) g = 1;
  return (uint32_t)g;
}

// split staging: begin allocates, chunk streams each input file's bytes
// as soon as its read completes (overlapping H2D with the remaining
// reads), finish uploads the block tables
int GpuJob::stage_begin(size_t blob_size, std::string* err) {
  Impl* p = p_;
  (void)hipEventRecord(p->stage_t0, p->stream);
  HIPCHK(p->d_blob_own.reserve(blob_size ? blob_size : 1));
  p->d_blob = p->d_blob_own;
  p->staged_split = true;
  return 0;
}
void GpuJob::stage_cancel() {
  Impl* p = p_;
  if (p->staged_split) {
    (void)hipStreamSynchronize(p->stream); // drain issued chunk copies
    p->staged_split = false;
  }
}

int GpuJob::stage_chunk(uint64_t off, const void* src, size_t n,
                        std::string* err) {
  Impl* p = p_;
  HIPCHK(hipMemcpyAsync(p->d_blob + off, src, n, hipMemcpyHostToDevice,
                        p->stream));
  return 0;
}

int GpuJob::stage(const GpuInputs& in, std::string* err) {
  Impl* p = p_;
  PhaseTimer t(p->stream, &ms_h2d);
  if (!p->staged_split) {
    HIPCHK(p->d_blob_own.reserve(in.blob_size));
    p->d_blob = p->d_blob_own;
    HIPCHK(hipMemcpyAsync(p->d_blob, in.blob, in.blob_size,
                          hipMemcpyHostToDevice, p->stream));
  }
  p->n_blocks = (uint32_t)in.blocks.size();
  p->checksum_type = in.checksum_type;
  std::vector<uint64_t> boff(p->n_blocks);
  std::vector<uint32_t> bsize(p->n_blocks);
  for (uint32_t i = 0; i < p->n_blocks; i++) {
    boff[i] = in.blocks[i].off;
    bsize[i] = in.blocks[i].size;
  }
  HIPCHK(p->d_boff_own.reserve(sizeof(uint64_t) * p->n_blocks));
  HIPCHK(p->d_bsize_own.reserve(sizeof(uint32_t) * p->n_blocks));
  p->d_boff = p->d_boff_own;
  p->d_bsize = p->d_bsize_own;
  HIPCHK(p->h2d_meta(p->d_boff, boff.data(), sizeof(uint64_t) * p->n_blocks));
  HIPCHK(p->h2d_meta(p->d_bsize, bsize.data(), sizeof(uint32_t) * p->n_blocks));
  if (p->arm_consts(err) != 0) return -1;
  t.stop();
  HIPCHK(hipStreamSynchronize(p->stream));
  // split staging started the clock at stage_begin
  t.add(p->staged_split ? (hipEvent_t)p->stage_t0 : nullptr);
  p->staged_split = false;
  // remember run boundaries (translated to entries later)
  run_blocks_ = in.run_block_begin;
  dzt_files_ = in.dzt_files;
  return 0;
}

StagedInput::~StagedInput() {
  if (d_blob) (void)hipFree(d_blob);
  if (d_boff) (void)hipFree(d_boff);
  if (d_bsize) (void)hipFree(d_bsize);
}

int GpuJob::stage_adopt(const StagedInput& s, std::string* err) {
  Impl* p = p_;
  p->d_blob = (uint8_t*)s.d_blob;
  p->d_boff = (uint64_t*)s.d_boff;
  p->d_bsize = (uint32_t*)s.d_bsize;
  p->n_blocks = s.n_blocks;
  p->checksum_type = s.checksum_type;
  run_blocks_ = s.run_block_begin;
  dzt_files_ = s.dzt_files;
  if (p->arm_consts(err) != 0) return -1;
  HIPCHK(hipStreamSynchronize(p->stream));
  return 0;
}

int GpuJob::stage_release(StagedInput* s, std::string* err) {
  Impl* p = p_;
  (void)err;
  // ownership of the staged buffers moves to the StagedInput; the job keeps
  // using them through the aliases, as borrowed
  s->d_blob = p->d_blob_own.release();
  s->d_boff = p->d_boff_own.release();
  s->d_bsize = p->d_bsize_own.release();
  s->n_blocks = p->n_blocks;
  s->checksum_type = p->checksum_type;
  s->run_block_begin = run_blocks_;
  s->dzt_files = dzt_files_;
  return 0;
}

int GpuJob::decode(std::string* err) {
  Impl* p = p_;
  PhaseTimer t(p->stream, &ms_decode);
  uint32_t nb = p->n_blocks;
  HIPCHK(p->d_usize.reserve(sizeof(uint32_t) * nb));
  HIPCHK(p->d_btype_in.reserve(nb));
  double in_block_bytes = 0; // filled below from bsize D2H; verify reads them
  // DZT inputs: a second class of blocks beside the BlockBasedTable ones;
  // each step below launches its DZT kernel right behind the existing one
  const bool has_dzt = !dzt_files_.empty();
  p->dzi_ulen_total = 0;
  if (has_dzt && dzt_upload_tables(err) != 0) return -1;
  const uint32_t n_dvb = has_dzt ? (uint32_t)p->h_dzi_vbs.size() : 0;
  p->kbegin("verify_checksum", 0);
  hipLaunchKernelGGL(k_verify_usize, dim3(grid_for(nb)), dim3(256), 0, p->stream,
                     p->d_blob, p->d_boff, p->d_bsize, nb, p->checksum_type,
                     p->d_crc, p->d_usize, p->d_btype_in, p->d_err);
  p->kend();
  if (n_dvb) {
    double stored = 0;
    for (auto& v : p->h_dzi_vbs) stored += v.csize + 5.0;
    p->kbegin("dzt_verify_vblocks", stored);
    hipLaunchKernelGGL(k_dzt_verify_vblocks, dim3(grid_for(n_dvb, 64)),
                       dim3(64), 0, p->stream, p->d_blob, p->d_dzi_vbs, n_dvb,
                       p->checksum_type, p->d_crc, p->d_dzi_btype, p->d_err);
    p->kend();
  }
  // host scan of usize -> uoff
  std::vector<uint32_t> usize(nb);
  HIPCHK(hipMemcpyAsync(usize.data(), p->d_usize, sizeof(uint32_t) * nb,
                        hipMemcpyDeviceToHost, p->stream));
  if (p->check_err("input block verify", err) != 0) return -1;
  std::vector<uint64_t> uoff(nb);
  uint64_t acc = 0;
  for (uint32_t i = 0; i < nb; i++) {
    uoff[i] = acc;
    acc += usize[i];
    in_block_bytes += usize[i]; // ~= compressed size; close enough for alg accounting
  }
  p->ublob_size = acc;
  HIPCHK(p->d_uoff.reserve(sizeof(uint64_t) * nb));
  HIPCHK(p->h2d_meta(p->d_uoff, uoff.data(), sizeof(uint64_t) * nb));
  p->dzi_ubase = acc; // decoded DZT value blocks follow the decoded BBT blocks
  HIPCHK(p->d_ublob.reserve(acc + p->dzi_ulen_total ? acc + p->dzi_ulen_total : 1));
  {
    std::lock_guard<std::mutex> lk(g_kmu);
    kstats()["verify_checksum"].alg_bytes += in_block_bytes;
  }
  static const int decomp_v =
      getenv("DCW_DECOMP_V") ? atoi(getenv("DCW_DECOMP_V")) : 0;
  p->kbegin("decompress", in_block_bytes + (double)acc);
  if (decomp_v == 1)
    hipLaunchKernelGGL(k_decompress_v1, dim3(grid_for(nb * 4ull)), dim3(256), 0,
                       p->stream, p->d_blob, p->d_boff, p->d_bsize,
                       p->d_btype_in, p->d_uoff, p->d_usize, nb, p->d_ublob,
                       p->d_err);
  else if (decomp_v == 2)
    hipLaunchKernelGGL(k_decompress_v2, dim3(grid_for(nb * 4ull)), dim3(256), 0,
                       p->stream, p->d_blob, p->d_boff, p->d_bsize,
                       p->d_btype_in, p->d_uoff, p->d_usize, nb, p->d_ublob,
                       p->d_err);
  else {
    static const uint32_t dec_pipe = [] {
      const char* v = getenv("DCW_DEC_PIPE");
      return (uint32_t)(v ? atoi(v) : 0);
    }();
    hipLaunchKernelGGL(k_decompress, dim3(grid_for(nb * 4ull)), dim3(256), 0,
                       p->stream, p->d_blob, p->d_boff, p->d_bsize,
                       p->d_btype_in, p->d_uoff, p->d_usize, nb, p->d_ublob,
                       p->d_err, dec_pipe);
  }
  p->kend();
  if (n_dvb) {
    double stored = 0;
    for (auto& v : p->h_dzi_vbs) stored += v.csize;
    p->kbegin("dzt_decompress", stored + (double)p->dzi_ulen_total);
    // one wave (one workgroup) per value block
    hipLaunchKernelGGL(k_dzt_decompress, dim3(n_dvb < 65536 ? n_dvb : 65536),
                       dim3(WAVE), 0, p->stream, p->d_blob, p->d_dzi_vbs,
                       p->d_dzi_files, p->d_dzi_btype, n_dvb,
                       p->d_ublob.get() + p->dzi_ubase, p->d_err);
    p->kend();
  }
  HIPCHK(p->d_nrestarts.reserve(sizeof(uint32_t) * nb));
  hipLaunchKernelGGL(k_num_restarts, dim3(grid_for(nb)), dim3(256), 0, p->stream,
                     p->d_ublob, p->d_uoff, p->d_usize, nb, p->d_nrestarts,
                     p->d_err);
  std::vector<uint32_t> nrestarts(nb);
  HIPCHK(hipMemcpyAsync(nrestarts.data(), p->d_nrestarts, sizeof(uint32_t) * nb,
                        hipMemcpyDeviceToHost, p->stream));
  if (p->check_err("block decompress/parse", err) != 0) return -1;
  // interval tables
  std::vector<uint32_t> iv_block, iv_local;
  std::vector<uint64_t> blk_iv_base(nb);
  uint64_t niv = 0;
  for (uint32_t b = 0; b < nb; b++) {
    blk_iv_base[b] = niv;
    for (uint32_t j = 0; j < nrestarts[b]; j++) {
      iv_block.push_back(b);
      iv_local.push_back(j);
    }
    niv += nrestarts[b];
  }
  p->n_intervals = (uint32_t)niv;
  HIPCHK(p->d_iv_block.reserve(sizeof(uint32_t) * niv));
  HIPCHK(p->d_iv_local.reserve(sizeof(uint32_t) * niv));
  HIPCHK(p->d_iv_cnt.reserve(sizeof(uint32_t) * niv));
  HIPCHK(p->d_iv_base.reserve(sizeof(uint32_t) * niv));
  HIPCHK(p->h2d_meta(p->d_iv_block, iv_block.data(), sizeof(uint32_t) * niv));
  HIPCHK(p->h2d_meta(p->d_iv_local, iv_local.data(), sizeof(uint32_t) * niv));
  p->kbegin("count_entries", (double)p->ublob_size);
  hipLaunchKernelGGL(k_count_entries, dim3(grid_for(niv)), dim3(256), 0, p->stream,
                     p->d_ublob, p->d_uoff, p->d_usize, p->d_nrestarts,
                     p->d_iv_block, p->d_iv_local, (uint32_t)niv, p->d_iv_cnt,
                     p->d_err);
  p->kend();
  std::vector<uint32_t> iv_cnt(niv);
  HIPCHK(hipMemcpyAsync(iv_cnt.data(), p->d_iv_cnt, sizeof(uint32_t) * niv,
                        hipMemcpyDeviceToHost, p->stream));
  if (p->check_err("entry count", err) != 0) return -1;
  std::vector<uint32_t> iv_base(niv);
  uint64_t total_entries = 0;
  for (uint64_t i = 0; i < niv; i++) {
    iv_base[i] = (uint32_t)total_entries;
    total_entries += iv_cnt[i];
  }
  p->n_entries = total_entries;
  n_entries_ = total_entries;
  // run entry boundaries
  p->run_entry_begin.clear();
  for (size_t r = 0; r + 1 < run_blocks_.size(); r++) {
    uint32_t first_blk = run_blocks_[r];
    p->run_entry_begin.push_back(first_blk < nb ? (first_blk == 0 ? 0 : iv_base[blk_iv_base[first_blk]])
                                                : total_entries);
  }
  p->run_entry_begin.push_back(total_entries);
  if (has_dzt) {
    // a run may mix both file kinds: lay the entry ranges out again in
    // run-major FILE order, each DZT file (n from its props) between the
    // BlockBasedTable blocks that blocks_before names
    std::vector<uint64_t> blk_cnt(nb, 0), blk_base(nb, 0);
    for (uint64_t i = 0; i < niv; i++) blk_cnt[iv_block[i]] += iv_cnt[i];
    p->run_entry_begin.clear();
    uint64_t pos = 0;
    size_t zi = 0, kb_row = 0;
    auto put_blocks = [&](uint32_t b0, uint32_t b1) {
      for (uint32_t b = b0; b < b1; b++) {
        blk_base[b] = pos;
        pos += blk_cnt[b];
      }
    };
    for (size_t r = 0; r + 1 < run_blocks_.size(); r++) {
      p->run_entry_begin.push_back(pos);
      uint32_t b = run_blocks_[r];
      for (; zi < dzt_files_.size() && dzt_files_[zi].run == r; zi++) {
        const DztFileRef& z = dzt_files_[zi];
        put_blocks(b, z.blocks_before);
        b = z.blocks_before;
        for (size_t k = 0; k < z.kblocks.size(); k++)
          p->h_dzi_kbs[kb_row++].out_base =
              (uint32_t)(pos + z.kblocks[k].first_rank);
        pos += z.n;
      }
      put_blocks(b, run_blocks_[r + 1]);
    }
    p->run_entry_begin.push_back(pos);
    if (pos > 0xfffffff0ull) {
      if (err) *err = "too many input entries";
      return -1;
    }
    uint32_t cur_blk = 0xffffffffu;
    uint64_t at = 0;
    for (uint64_t i = 0; i < niv; i++) {
      if (iv_block[i] != cur_blk) {
        cur_blk = iv_block[i];
        at = blk_base[cur_blk];
      }
      iv_base[i] = (uint32_t)at;
      at += iv_cnt[i];
    }
    total_entries = pos;
    p->n_entries = total_entries;
    n_entries_ = total_entries;
  }
  HIPCHK(p->h2d_meta(p->d_iv_base, iv_base.data(), sizeof(uint32_t) * niv));
  HIPCHK(p->d_ent[0].reserve(sizeof(ulong4) * total_entries));
  HIPCHK(p->d_ent[1].reserve(sizeof(ulong4) * total_entries));
  HIPCHK(p->d_voff.reserve(sizeof(uint64_t) * total_entries));
  HIPCHK(p->d_vlen.reserve(sizeof(uint32_t) * total_entries));
  HIPCHK(p->d_klen.reserve(total_entries));
  p->kbegin("decode_entries", (double)p->ublob_size + 45.0 * total_entries);
  hipLaunchKernelGGL(k_decode_entries, dim3(grid_for(niv)), dim3(256), 0,
                     p->stream, p->d_ublob, p->d_uoff, p->d_usize, p->d_nrestarts,
                     p->d_iv_block, p->d_iv_local, p->d_iv_base, (uint32_t)niv,
                     p->d_ent[0], p->d_voff, p->d_vlen, p->d_klen,
                     p->d_uklen_probe, p->d_err);
  p->kend();
  uint32_t uklen = 0, code = 0;
  HIPCHK(hipMemcpyAsync(&uklen, p->d_uklen_probe, 4, hipMemcpyDeviceToHost,
                        p->stream));
  // no message yet: DE_UKEY_LEN is not a failure but the cue to retry
  if (p->check_err(nullptr, err, &code, &t) != 0) return -1;
  // DZT files state their key length in the props, so their mode is known
  // before their key kernel runs (once, in the right mode): fast only when
  // every DZT file and every BlockBasedTable entry share one U <= 16
  bool dzt_general = false;
  if (has_dzt) {
    uint32_t zu = dzt_files_[0].ukey_len;
    for (auto& z : dzt_files_) dzt_general |= z.ukey_len != zu;
    dzt_general |= zu > 16 || (uklen != 0xffffffffu && uklen != zu);
    if (!dzt_general) uklen = zu;
  }
  if (code == DE_UKEY_LEN || (code == DE_OK && dzt_general)) {
    // GENERAL-KEY retry: mixed lengths / 16 < ukey <= DCW_GKEY_MAX via the
    // prefix normkey + full-key side table (arbitrary-length bytewise
    // contract, db/dbformat.h:1057-1096)
    PhaseTimer g(p->stream, &ms_decode);
    HIPCHK(hipMemsetAsync(p->d_err, 0, 8, p->stream));
    HIPCHK(p->d_kext.reserve((uint64_t)total_entries * 48u + 64));
    p->kbegin("decode_entries_g",
              (double)p->ublob_size + 93.0 * total_entries);
    hipLaunchKernelGGL(k_decode_entries_g, dim3(grid_for(niv)), dim3(256), 0,
                       p->stream, p->d_ublob, p->d_uoff, p->d_usize,
                       p->d_nrestarts, p->d_iv_block, p->d_iv_local,
                       p->d_iv_base, (uint32_t)niv, p->d_ent[0], p->d_voff,
                       p->d_vlen, p->d_klen, p->d_kext, p->d_err);
    p->kend();
    if (p->check_err("general-key decode", err, &code, &g) != 0) {
      if (err && code == DE_UKEY_LEN) *err += " (user key > 48 B)";
      return -1;
    }
    general_keys = true;
    ukey_len = 0;
    return has_dzt ? dzt_decode_keys(true, err) : 0;
  }
  if (code) {
    if (err) *err = "entry decode failed, code " + std::to_string(code);
    return -1;
  }
  ukey_len = uklen;
  return has_dzt ? dzt_decode_keys(false, err) : 0;
}

// Build the flat DZT tables from the parsed files and upload them.  Every
// offset was bounds-checked against its section by parse_dzt.
int GpuJob::dzt_upload_tables(std::string* err) {
  Impl* p = p_;
  p->h_dzi_vbs.clear();
  p->h_dzi_kbs.clear();
  std::vector<DztFileIn> files;
  uint64_t uoff = 0;
  for (size_t fi = 0; fi < dzt_files_.size(); fi++) {
    const DztFileRef& z = dzt_files_[fi];
    const uint32_t vb0 = (uint32_t)p->h_dzi_vbs.size();
    for (auto& v : z.vblocks) {
      DztVbIn row;
      row.off = z.value_off + v.voff;
      row.uoff = uoff;
      row.csize = v.csize;
      row.ulen = v.ulen;
      row.first_rank = (uint32_t)v.first_rank;
      row.file = (uint32_t)fi;
      p->h_dzi_vbs.push_back(row);
      uoff += v.ulen;
    }
    size_t vb = 0; // value block holding each key block's first rank
    for (size_t k = 0; k < z.kblocks.size(); k++) {
      const DztKeyIndexEntry& e = z.kblocks[k];
      while (vb + 1 < z.vblocks.size() && z.vblocks[vb + 1].first_rank <= e.first_rank)
        vb++;
      uint64_t next = k + 1 < z.kblocks.size() ? z.kblocks[k + 1].first_rank : z.n;
      DztKbIn row;
      row.off = z.key_off + e.koff;
      row.kidx_off = z.kindex_off + k * ((uint64_t)z.ukey_len + 28);
      row.ksize = e.ksize;
      row.count = (uint32_t)(next - e.first_rank);
      row.first_rank = (uint32_t)e.first_rank;
      row.out_base = 0;
      row.vb_start = vb0 + (uint32_t)vb;
      row.file = (uint32_t)fi;
      row.has_next = k + 1 < z.kblocks.size();
      row.pad = 0;
      p->h_dzi_kbs.push_back(row);
    }
    DztFileIn f;
    f.dict_off = z.dict_off;
    f.dict_size = z.dict_size;
    f.U = z.ukey_len;
    f.vb_end = (uint32_t)p->h_dzi_vbs.size();
    f.pad = 0;
    files.push_back(f);
  }
  p->dzi_ulen_total = uoff;
  size_t nvb = p->h_dzi_vbs.size();
  HIPCHK(p->d_dzi_vbs.reserve(sizeof(DztVbIn) * nvb));
  HIPCHK(p->d_dzi_files.reserve(sizeof(DztFileIn) * files.size()));
  HIPCHK(p->d_dzi_btype.reserve(nvb));
  HIPCHK(p->h2d_meta(p->d_dzi_vbs, p->h_dzi_vbs.data(), sizeof(DztVbIn) * nvb));
  HIPCHK(p->h2d_meta(p->d_dzi_files, files.data(), sizeof(DztFileIn) * files.size()));
  return 0;
}

// Key-block decode of every DZT file into the shared entry arrays; runs
// behind the BlockBasedTable entry decode, in the mode decode() settled.
int GpuJob::dzt_decode_keys(bool general, std::string* err) {
  Impl* p = p_;
  PhaseTimer t(p->stream, &ms_decode);
  uint32_t nkb = (uint32_t)p->h_dzi_kbs.size();
  HIPCHK(p->d_dzi_kbs.reserve(sizeof(DztKbIn) * nkb));
  HIPCHK(p->h2d_meta(p->d_dzi_kbs, p->h_dzi_kbs.data(), sizeof(DztKbIn) * nkb));
  double key_bytes = 0, ents = 0;
  for (auto& k : p->h_dzi_kbs) {
    key_bytes += k.ksize;
    ents += k.count;
  }
  p->kbegin("dzt_decode_keys", key_bytes + (general ? 93.0 : 45.0) * ents);
  hipLaunchKernelGGL(k_dzt_decode_keys, dim3(grid_for(nkb, 64)), dim3(64), 0,
                     p->stream, p->d_blob, p->d_dzi_kbs, nkb, p->d_dzi_vbs,
                     p->d_dzi_files, p->dzi_ubase, general ? 1 : 0, p->d_ent[0],
                     p->d_voff, p->d_vlen, p->d_klen, p->d_kext, p->d_err);
  p->kend();
  uint32_t code = 0;
  if (p->check_err("DZT key decode", err, &code, &t) != 0) return -1;
  return 0;
}

int GpuJob::decode_flush(const dcw_job_desc* d, std::string* err) {
  Impl* p = p_;
  uint64_t n = d->flush_num_entries;
  // host pre-scan of record key lengths: pick fast vs general mode and
  // validate bounds (the blob is caller host memory)
  bool general = false;
  uint32_t ulen0 = 0;
  for (uint64_t i = 0; i < n; i++) {
    uint32_t klen;
    if (d->flush_offsets[i] + 8 > d->flush_kv_bytes) {
      if (err) *err = "flush record out of bounds";
      return -1;
    }
    memcpy(&klen, d->flush_kv + d->flush_offsets[i], 4);
    if (klen < 9 || klen > DCW_GKEY_MAX + 8u) {
      if (err) *err = "flush key length outside envelope";
      return -1;
    }
    uint32_t ul = klen - 8;
    if (i == 0) ulen0 = ul;
    if (ul != ulen0 || ul > 16) general = true;
  }
  PhaseTimer t(p->stream, &ms_decode);
  HIPCHK(p->d_ublob.reserve(d->flush_kv_bytes + 64));
  p->ublob_size = d->flush_kv_bytes;
  HIPCHK(hipMemcpyAsync(p->d_ublob, d->flush_kv, d->flush_kv_bytes,
                        hipMemcpyHostToDevice, p->stream));
  HIPCHK(p->d_flush_offs.reserve((n + 1) * 8));
  HIPCHK(hipMemcpyAsync(p->d_flush_offs, d->flush_offsets, (n + 1) * 8,
                        hipMemcpyHostToDevice, p->stream));
  if (p->arm_consts(err) != 0) return -1;
  HIPCHK(p->d_ent[0].reserve(sizeof(ulong4) * (n + 1)));
  HIPCHK(p->d_ent[1].reserve(sizeof(ulong4) * (n + 1)));
  HIPCHK(p->d_voff.reserve(sizeof(uint64_t) * (n + 1)));
  HIPCHK(p->d_vlen.reserve(sizeof(uint32_t) * (n + 1)));
  HIPCHK(p->d_klen.reserve(n + 1));
  if (general) HIPCHK(p->d_kext.reserve(n * 48ull + 64));
  p->kbegin("decode_flush", (double)d->flush_kv_bytes + 45.0 * n);
  hipLaunchKernelGGL(k_decode_flush, dim3(grid_for(n)), dim3(256), 0,
                     p->stream, p->d_ublob, p->d_flush_offs,
                     n, general ? 1 : 0, ulen0, p->d_ent[0], p->d_voff,
                     p->d_vlen, p->d_klen, p->d_kext, p->d_err);
  p->kend();
  if (p->check_err("flush decode", err, nullptr, &t) != 0) return -1;
  p->n_entries = n;
  n_entries_ = n;
  p->run_entry_begin.clear();
  p->run_entry_begin.push_back(0);
  p->run_entry_begin.push_back(n);
  p->final_buf = 0;
  general_keys = general;
  ukey_len = general ? 0 : ulen0;
  return 0;
}

int GpuJob::merge(std::string* err) {
  Impl* p = p_;
  PhaseTimer t(p->stream, &ms_merge);
  std::vector<uint64_t> bounds = p->run_entry_begin; // size k+1
  int cur = 0;
  // tile-boundary scratch shared by every pair (launches on one stream
  // serialize, so no pair's diags outlive its own merge launch); env
  // DCW_MERGE_V=0 falls back to in-kernel thread-0 searches
  static const bool diag_precompute = [] {
    const char* v = getenv("DCW_MERGE_V");
    return !v || atoi(v) != 0;
  }();
  if (diag_precompute && bounds.size() > 2)
    HIPCHK(p->d_merge_diag.reserve(sizeof(uint64_t) * (bounds.back() / MT_TILE + 2)));
  while (bounds.size() > 2) {
    std::vector<uint64_t> nbounds;
    nbounds.push_back(0);
    size_t k = bounds.size() - 1;
    for (size_t i = 0; i + 1 < k; i += 2) {
      uint64_t a0 = bounds[i], a1 = bounds[i + 1], b1 = bounds[i + 2];
      uint64_t nA = a1 - a0, nB = b1 - a1;
      uint64_t ntiles = (nA + nB + MT_TILE - 1) / MT_TILE;
      const uint64_t* diags = nullptr;
      if (diag_precompute) {
        hipLaunchKernelGGL(k_merge_diags,
                           dim3((uint32_t)((ntiles + 256) / 256)), dim3(256), 0,
                           p->stream, p->d_ent[cur] + a0, nA,
                           p->d_ent[cur] + a1, nB,
                           general_keys ? p->d_kext.get() : nullptr,
                           p->d_klen, ntiles, p->d_merge_diag);
        diags = p->d_merge_diag;
      }
      p->kbegin("merge_pair", 64.0 * (double)(nA + nB));
      hipLaunchKernelGGL(k_merge_tiled,
                         dim3((uint32_t)(ntiles < 8192 ? ntiles : 8192)),
                         dim3(MT_TPB), 0, p->stream, p->d_ent[cur] + a0, nA,
                         p->d_ent[cur] + a1, nB, p->d_ent[cur ^ 1] + a0,
                         general_keys ? p->d_kext.get() : nullptr,
                         p->d_klen, diags);
      p->kend();
      nbounds.push_back(b1);
    }
    if (k % 2) { // odd leftover run: copy through
      uint64_t a0 = bounds[k - 1], a1 = bounds[k];
      HIPCHK(hipMemcpyAsync(p->d_ent[cur ^ 1] + a0, p->d_ent[cur] + a0,
                            sizeof(ulong4) * (a1 - a0), hipMemcpyDeviceToDevice,
                            p->stream));
      nbounds.push_back(a1);
    }
    bounds.swap(nbounds);
    cur ^= 1;
  }
  p->final_buf = cur;
  t.stop();
  HIPCHK(hipStreamSynchronize(p->stream));
  t.add();
  p->kresolve();
  return 0;
}

// device exclusive scan of a u8 array into u32 positions; returns total
static int scan_u8(GpuJob::Impl* p, const uint8_t* d_in, uint64_t n,
                   uint32_t* d_out, uint64_t* total, std::string* err) {
  uint64_t nblk = (n + 1023) / 1024;
  HIPCHK(p->d_scan_bs.reserve(sizeof(uint32_t) * (nblk + 1)));
  uint32_t* d_bs = p->d_scan_bs;
  hipLaunchKernelGGL(k_scan_partial, dim3((uint32_t)nblk), dim3(1024), 0,
                     p->stream, d_in, n, d_out, d_bs);
  std::vector<uint32_t> bs(nblk);
  HIPCHK(hipMemcpyAsync(bs.data(), d_bs, sizeof(uint32_t) * nblk,
                        hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  uint64_t acc = 0;
  for (uint64_t i = 0; i < nblk; i++) {
    uint32_t v = bs[i];
    bs[i] = (uint32_t)acc;
    acc += v;
  }
  HIPCHK(p->h2d_meta(d_bs, bs.data(), sizeof(uint32_t) * nblk));
  hipLaunchKernelGGL(k_scan_add_base, dim3((uint32_t)nblk), dim3(1024), 0,
                     p->stream, d_out, n, d_bs);
  // `bs` is a local: the async H2D must complete before it dies (ROCm may
  // read pageable sources lazily at stream-execution time)
  HIPCHK(hipStreamSynchronize(p->stream));
  *total = acc;
  return 0;
}

int GpuJob::dedup(const dcw_job_desc* d, std::string* err) {
  Impl* p = p_;
  PhaseTimer t(p->stream, &ms_dedup);
  uint64_t n = p->n_entries;
  const ulong4* ents = p->d_ent[p->final_buf];
  HIPCHK(p->d_head.reserve(n));
  p->kbegin("mark_heads", 17.0 * n);
  hipLaunchKernelGGL(k_mark_heads, dim3(grid_for(n)), dim3(256), 0, p->stream,
                     ents, n,
                     general_keys ? p->d_kext.get() : nullptr,
                     p->d_klen, p->d_head);
  p->kend();
  // head positions via scan, then gather head indices on host
  HIPCHK(p->d_pos.reserve(sizeof(uint32_t) * n));
  uint64_t ngroups = 0;
  if (scan_u8(p, p->d_head, n, p->d_pos, &ngroups, err) != 0) return -1;
  p->n_groups = ngroups;
  // build head_idx on device: head[i] -> headidx[pos[i]] = i
  HIPCHK(p->d_headidx.reserve(sizeof(uint64_t) * (ngroups ? ngroups : 1)));
  hipLaunchKernelGGL(k_build_headidx, dim3(grid_for(n)), dim3(256), 0, p->stream,
                     p->d_head, p->d_pos, n, p->d_headidx);
  // FSM params
  FsmParams P;
  memset(&P, 0, sizeof(P));
  P.num_snapshots = d->num_snapshots;
  P.visible_at_tip = d->num_snapshots == 0;
  P.earliest_snapshot = d->num_snapshots ? d->snapshots[0] : kMaxSeq;
  P.ewcs = d->earliest_write_conflict_snapshot;
  P.bottommost = d->bottommost_level ? 1 : 0;
  P.levels_below_valid = d->levels_below_valid ? 1 : 0;
  if (d->num_snapshots) {
    HIPCHK(p->d_snaps.reserve(sizeof(uint64_t) * d->num_snapshots));
    HIPCHK(p->h2d_meta(p->d_snaps, d->snapshots, sizeof(uint64_t) * d->num_snapshots));
    P.snapshots = p->d_snaps;
  }
  // levels below -> normkeys (the 16-byte prefix) + true lengths; in
  // general-key mode also the boundary bytes a <= 48 B job key can reach
  std::vector<uint64_t> sm0, sm1, lg0, lg1;
  std::vector<uint32_t> smlen, lglen;
  std::vector<uint8_t> smext, lgext;
  std::vector<uint32_t> lbeg{0};
  auto add_bound = [&](const uint8_t* k, uint32_t len, std::vector<uint64_t>& w0,
                       std::vector<uint64_t>& w1, std::vector<uint32_t>& lens,
                       std::vector<uint8_t>& ext) {
    uint64_t a, b, c;
    make_normkey(k, len, 0, &a, &b, &c);
    w0.push_back(a);
    w1.push_back(b);
    lens.push_back(len);
    if (general_keys) {
      size_t at = ext.size();
      ext.resize(at + DCW_GKEY_STRIDE, 0);
      memcpy(ext.data() + at, k, len < DCW_GKEY_MAX ? len : DCW_GKEY_MAX);
    }
  };
  for (uint32_t l = 0; l < d->num_levels_below; l++) {
    const dcw_level_files* lf = &d->levels_below[l];
    for (uint32_t f = 0; f < lf->num_files; f++) {
      add_bound(lf->files[f].smallest_ukey, lf->files[f].smallest_len, sm0, sm1,
                smlen, smext);
      add_bound(lf->files[f].largest_ukey, lf->files[f].largest_len, lg0, lg1,
                lglen, lgext);
    }
    lbeg.push_back((uint32_t)sm0.size());
  }
  P.num_levels = d->num_levels_below;
  if (!sm0.empty()) {
    size_t nb = sm0.size() * 8;
    HIPCHK(p->d_lb_sm0.reserve(nb));
    HIPCHK(p->d_lb_sm1.reserve(nb));
    HIPCHK(p->d_lb_lg0.reserve(nb));
    HIPCHK(p->d_lb_lg1.reserve(nb));
    HIPCHK(p->d_lb_smlen.reserve(nb / 2));
    HIPCHK(p->d_lb_lglen.reserve(nb / 2));
    HIPCHK(p->h2d_meta(p->d_lb_sm0, sm0.data(), nb));
    HIPCHK(p->h2d_meta(p->d_lb_sm1, sm1.data(), nb));
    HIPCHK(p->h2d_meta(p->d_lb_lg0, lg0.data(), nb));
    HIPCHK(p->h2d_meta(p->d_lb_lg1, lg1.data(), nb));
    HIPCHK(p->h2d_meta(p->d_lb_smlen, smlen.data(), nb / 2));
    HIPCHK(p->h2d_meta(p->d_lb_lglen, lglen.data(), nb / 2));
    P.lb_sm_len = p->d_lb_smlen;
    P.lb_lg_len = p->d_lb_lglen;
    if (general_keys) {
      HIPCHK(p->d_lb_smext.reserve(smext.size()));
      HIPCHK(p->d_lb_lgext.reserve(lgext.size()));
      HIPCHK(p->h2d_meta(p->d_lb_smext, smext.data(), smext.size()));
      HIPCHK(p->h2d_meta(p->d_lb_lgext, lgext.data(), lgext.size()));
      P.lb_sm_ext = p->d_lb_smext;
      P.lb_lg_ext = p->d_lb_lgext;
    }
  }
  if (general_keys) {
    P.kext = p->d_kext;
    P.klen = p->d_klen;
  }
  HIPCHK(p->d_lb_beg.reserve(sizeof(uint32_t) * lbeg.size()));
  HIPCHK(p->h2d_meta(p->d_lb_beg, lbeg.data(), sizeof(uint32_t) * lbeg.size()));
  P.lb_sm_k0 = p->d_lb_sm0;
  P.lb_sm_k1 = p->d_lb_sm1;
  P.lb_lg_k0 = p->d_lb_lg0;
  P.lb_lg_k1 = p->d_lb_lg1;
  P.lb_level_beg = p->d_lb_beg;
  // range-deletion fragments
  P.num_rd = (uint32_t)rd_frags_.size();
  P.rd_ukey_len = ukey_len;
  if (P.num_rd) {
    std::vector<uint64_t> fk0(P.num_rd), fk1(P.num_rd), fsq(P.num_rd);
    std::vector<uint32_t> fln(P.num_rd);
    for (uint32_t i = 0; i < P.num_rd; i++) {
      fk0[i] = rd_frags_[i].k0;
      fk1[i] = rd_frags_[i].k1;
      fln[i] = rd_frags_[i].len;
      fsq[i] = rd_frags_[i].max_seq;
    }
    HIPCHK(p->d_rd_k0.reserve(P.num_rd * 8));
    HIPCHK(p->d_rd_k1.reserve(P.num_rd * 8));
    HIPCHK(p->d_rd_len.reserve(P.num_rd * 4));
    HIPCHK(p->d_rd_seq.reserve(P.num_rd * 8));
    HIPCHK(p->h2d_meta(p->d_rd_k0, fk0.data(), P.num_rd * 8));
    HIPCHK(p->h2d_meta(p->d_rd_k1, fk1.data(), P.num_rd * 8));
    HIPCHK(p->h2d_meta(p->d_rd_len, fln.data(), P.num_rd * 4));
    HIPCHK(p->h2d_meta(p->d_rd_seq, fsq.data(), P.num_rd * 8));
    P.rd_k0 = p->d_rd_k0;
    P.rd_k1 = p->d_rd_k1;
    P.rd_len = p->d_rd_len;
    P.rd_seq = p->d_rd_seq;
    if (general_keys) {
      std::vector<uint8_t> fext((size_t)P.num_rd * DCW_GKEY_STRIDE);
      for (uint32_t i = 0; i < P.num_rd; i++)
        memcpy(fext.data() + (size_t)i * DCW_GKEY_STRIDE, rd_frags_[i].ext,
               DCW_GKEY_STRIDE);
      HIPCHK(p->d_rd_ext.reserve(fext.size()));
      HIPCHK(p->h2d_meta(p->d_rd_ext, fext.data(), fext.size()));
      P.rd_ext = p->d_rd_ext;
    }
  }

  HIPCHK(p->d_survive.reserve(n));
  HIPCHK(p->d_newtag.reserve(sizeof(uint64_t) * n));
  HIPCHK(p->d_clearv.reserve(n));
  HIPCHK(p->d_gflags.reserve(ngroups ? ngroups : 1));
  // entries skipped by multi-consume FSM paths never store their slot:
  // they must read as "dropped"
  HIPCHK(hipMemsetAsync(p->d_survive, 0, n, p->stream));
  HIPCHK(hipMemsetAsync(p->d_clearv, 0, n, p->stream));
  p->kbegin("group_fsm", 42.0 * n);
  hipLaunchKernelGGL(k_group_fsm, dim3(grid_for(ngroups)), dim3(256), 0,
                     p->stream, ents, n, p->d_headidx, ngroups, P, p->d_survive,
                     p->d_newtag, p->d_clearv, p->d_gflags, ~0ull, p->d_err);
  p->kend();
  // SeekToFirst lag: re-run the first group that produced output if its SD
  // decisions were has_outputted-sensitive
  std::vector<uint8_t> gflags(ngroups);
  HIPCHK(hipMemcpyAsync(gflags.data(), p->d_gflags, ngroups,
                        hipMemcpyDeviceToHost, p->stream));
  if (p->check_err("dedup FSM", err) != 0) return -1;
  bool lag_ran = false;
  for (uint64_t g = 0; g < ngroups; g++) {
    if (gflags[g] & GF_PRODUCED) {
      if (gflags[g] & GF_LAG_SENSITIVE) {
        hipLaunchKernelGGL(k_group_fsm, dim3(1), dim3(64), 0, p->stream, ents, n,
                           p->d_headidx, ngroups, P, p->d_survive, p->d_newtag,
                           p->d_clearv, (uint8_t*)nullptr, g, p->d_err);
        lag_ran = true;
      }
      break;
    }
  }
  // a DE_SD_CONTRACT/DE_TYPE from the rerun must fail the job
  if (lag_ran && p->check_err("dedup FSM (lag rerun)", err) != 0) return -1;
  // survivor compaction
  uint64_t nsurv = 0;
  if (scan_u8(p, p->d_survive, n, p->d_pos, &nsurv, err) != 0) return -1;
  p->n_surv = nsurv;
  n_surv_ = nsurv;
  HIPCHK(p->d_sk0.reserve(sizeof(uint64_t) * (nsurv + 1)));
  HIPCHK(p->d_sk1.reserve(sizeof(uint64_t) * (nsurv + 1)));
  HIPCHK(p->d_stag.reserve(sizeof(uint64_t) * (nsurv + 1)));
  HIPCHK(p->d_svoff.reserve(sizeof(uint64_t) * (nsurv + 1)));
  HIPCHK(p->d_svlen.reserve(sizeof(uint32_t) * (nsurv + 1)));
  HIPCHK(p->d_sklen.reserve(nsurv + 1));
  HIPCHK(p->d_sshared.reserve(nsurv + 1));
  HIPCHK(p->d_sw.reserve(sizeof(uint32_t) * (nsurv + 1)));
  p->kbegin("gather_survivors", 90.0 * n);
  hipLaunchKernelGGL(k_gather_survivors, dim3(grid_for(n)), dim3(256), 0,
                     p->stream, ents, n, p->d_survive, p->d_pos, p->d_newtag,
                     p->d_clearv, p->d_voff, p->d_vlen, p->d_klen, p->d_sk0,
                     p->d_sk1, p->d_stag, p->d_svoff, p->d_svlen, p->d_sklen,
                     p->d_sw);
  p->kend();
  p->kbegin("shared_prefix", 50.0 * nsurv);
  hipLaunchKernelGGL(k_shared_prefix, dim3(grid_for(nsurv)), dim3(256), 0,
                     p->stream, p->d_sk0, p->d_sk1, p->d_stag, p->d_sklen, nsurv,
                     general_keys ? p->d_kext.get() : nullptr,
                     p->d_sw, p->d_sshared);
  p->kend();
  // plan metadata D2H
  h_shared_.resize(nsurv);
  h_klen_.resize(nsurv);
  h_vlen_.resize(nsurv);
  if (nsurv) {
    HIPCHK(hipMemcpyAsync(h_shared_.data(), p->d_sshared, nsurv,
                          hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipMemcpyAsync(h_klen_.data(), p->d_sklen, nsurv,
                          hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipMemcpyAsync(h_vlen_.data(), p->d_svlen, sizeof(uint32_t) * nsurv,
                          hipMemcpyDeviceToHost, p->stream));
  }
  t.stop();
  HIPCHK(hipStreamSynchronize(p->stream));
  t.add();
  p->kresolve();
  return 0;
}

int GpuJob::plan_all(const TableOpts& o, const uint32_t** next,
                     const uint32_t** unc, const uint16_t** nrst,
                     std::string* err) {
  Impl* p = p_;
  uint64_t n = p->n_surv;
  // pinned host landing buffers (grow-only): next u32 + unc u32 + nr u16
  HIPCHK(p->h_plan.reserve(n * 10, /*allow_pageable=*/true));
  uint32_t* h_next = (uint32_t*)p->h_plan.get();
  uint32_t* h_unc = h_next + n;
  uint16_t* h_nr = (uint16_t*)(h_unc + n);
  HIPCHK(p->d_plan_next.reserve(n * 4 + 4));
  HIPCHK(p->d_plan_meta.reserve(n * 4 + 4));
  HIPCHK(p->d_plan_nr.reserve(n * 2 + 4));
  uint64_t dev_limit =
      ((o.block_size * (100 - o.block_size_deviation)) + 99) / 100;
  p->kbegin("plan_next", 40.0 * n);
  hipLaunchKernelGGL(k_plan_next, dim3(grid_for(n)), dim3(256), 0, p->stream,
                     p->d_sshared, p->d_sklen, p->d_svlen, n, o.block_size,
                     o.block_restart_interval, dev_limit,
                     p->d_plan_next, p->d_plan_meta,
                     p->d_plan_nr, p->d_err);
  p->kend();
  HIPCHK(hipMemcpyAsync(h_next, p->d_plan_next, n * 4, hipMemcpyDeviceToHost,
                        p->stream));
  HIPCHK(hipMemcpyAsync(h_unc, p->d_plan_meta, n * 4, hipMemcpyDeviceToHost,
                        p->stream));
  HIPCHK(hipMemcpyAsync(h_nr, p->d_plan_nr, n * 2, hipMemcpyDeviceToHost,
                        p->stream));
  uint32_t code = 0;
  int rc = p->check_err("block plan", err, &code);
  p->kresolve();
  if (rc != 0) {
    if (err && code == DE_PLAN_WIDTH)
      *err += " (block shape exceeds the emit envelope)";
    return -1;
  }
  *next = h_next;
  *unc = h_unc;
  *nrst = h_nr;
  return 0;
}

int GpuJob::emit_blocks(const std::vector<PlannedBlock>& blocks, const TableOpts& o,
                        std::vector<uint32_t>* comp_sizes, std::string* err) {
  Impl* p = p_;
  PhaseTimer t(p->stream, &ms_emit);
  uint32_t nb = (uint32_t)blocks.size();
  if (nb == 0) {
    comp_sizes->clear();
    return 0;
  }
  // per-entry in-block offsets + block descs
  uint64_t first = blocks.front().first;
  uint64_t last = blocks.back().first + blocks.back().count;
  uint64_t nent = last - first;
  (void)nent;
  // descs: raw-image offsets (uout) and, for snappy output, every block's
  // own compressed-output slot (cout): a running sum of worst-case encoder
  // sizes, so one huge block does not size every slot of the chunk.  Blocks
  // over SNAP_MAX_UNC are listed for k_compress_large.
  std::vector<EmitBlockDesc> bds(nb);
  std::vector<uint32_t> big;
  uint64_t uout = 0, cslot = 0;
  for (uint32_t b = 0; b < nb; b++) {
    const PlannedBlock& pb = blocks[b];
    bds[b] = {(uint32_t)pb.first, pb.count, pb.unc_size, pb.num_restarts, uout,
              cslot};
    uout += pb.unc_size;
    if (o.compression == 1) {
      if (pb.unc_size > SNAP_LARGE_MAX_UNC) {
        if (err)
          *err = "data block of " + std::to_string(pb.unc_size) +
                 " B is past the snappy encoder's 2 GiB bound; job outside "
                 "envelope";
        return -1;
      }
      cslot += (snappy_max_compressed(pb.unc_size) + 63) & ~(uint64_t)63;
      if (pb.unc_size > SNAP_MAX_UNC) big.push_back(b);
    }
  }
  p->emit_base = first;
  p->emit_nblocks = nb;
  HIPCHK(p->d_bds.reserve(sizeof(EmitBlockDesc) * nb));
  HIPCHK(p->d_ucblob.reserve(uout));
  HIPCHK(p->d_ebsize.reserve(sizeof(uint32_t) * nb * 2 + nb)); // bsize+csum+btype
  p->d_ecsum = p->d_ebsize + nb;
  p->d_ebtype = (uint8_t*)(p->d_ecsum + nb);
  HIPCHK(p->h2d_meta(p->d_bds, bds.data(), sizeof(EmitBlockDesc) * nb));
  p->kbegin("emit", 2.0 * (double)uout);
  hipLaunchKernelGGL(k_emit, dim3(nb < 4096 ? nb : 4096), dim3(256), 0, p->stream,
                     p->d_bds, nb, p->d_sk0, p->d_sk1, p->d_stag, p->d_svoff,
                     p->d_svlen, p->d_sklen, p->d_sshared, p->d_ublob,
                     p->d_ucblob, o.block_restart_interval,
                     general_keys ? p->d_kext.get() : nullptr,
                     p->d_sw, p->d_err);
  p->kend();
  if (o.compression == 1) {
    HIPCHK(p->d_cblob.reserve(cslot));
    // DCW_COMPRESS_V picks the kernel for blocks up to SNAP_MAX_UNC only
    // (0 default, 1/2/3 the re-verification variants of DESIGN §5); each of
    // them skips a larger block, which k_compress_large encodes the same
    // way under every value
    static const int comp_v =
        getenv("DCW_COMPRESS_V") ? atoi(getenv("DCW_COMPRESS_V")) : 0;
    p->kbegin("compress", 1.6 * (double)uout);
    uint32_t cgrid = (nb + 3) / 4;
    if (comp_v == 1)
      hipLaunchKernelGGL(k_compress_ldsin, dim3(cgrid < 4096 ? cgrid : 4096),
                         dim3(256), 0, p->stream, p->d_bds, nb, p->d_ucblob,
                         p->d_cblob, p->d_ebsize, p->d_ebtype);
    else if (comp_v == 2)
      hipLaunchKernelGGL(k_compress_2p<1>, dim3(cgrid < 4096 ? cgrid : 4096),
                         dim3(256), 0, p->stream, p->d_bds, nb, p->d_ucblob,
                         p->d_cblob, p->d_ebsize, p->d_ebtype);
    else if (comp_v == 3)
      hipLaunchKernelGGL(k_compress_2p<0>, dim3(cgrid < 4096 ? cgrid : 4096),
                         dim3(256), 0, p->stream, p->d_bds, nb, p->d_ucblob,
                         p->d_cblob, p->d_ebsize, p->d_ebtype);
    else
      hipLaunchKernelGGL(k_compress, dim3(cgrid < 4096 ? cgrid : 4096),
                         dim3(256), 0, p->stream, p->d_bds, nb, p->d_ucblob,
                         p->d_cblob, p->d_ebsize, p->d_ebtype);
    p->kend();
    if (!big.empty()) {
      uint32_t nbig = (uint32_t)big.size();
      uint64_t big_unc = 0;
      for (uint32_t b : big) big_unc += blocks[b].unc_size;
      HIPCHK(p->d_bigidx.reserve(sizeof(uint32_t) * nbig));
      HIPCHK(p->h2d_meta(p->d_bigidx, big.data(), sizeof(uint32_t) * nbig));
      p->kbegin("compress_large", 1.6 * (double)big_unc);
      uint32_t lgrid = (nbig + 3) / 4;
      hipLaunchKernelGGL(k_compress_large, dim3(lgrid < 4096 ? lgrid : 4096),
                         dim3(256), 0, p->stream, p->d_bds, p->d_bigidx, nbig,
                         p->d_ucblob, p->d_cblob, p->d_ebsize, p->d_ebtype,
                         p->d_err);
      p->kend();
    }
  } else {
    hipLaunchKernelGGL(k_sizes_nocomp, dim3(grid_for(nb)), dim3(256), 0,
                       p->stream, p->d_bds, nb, p->d_ebsize, p->d_ebtype);
  }
  p->kbegin("checksum", (double)uout);
  hipLaunchKernelGGL(k_checksum, dim3(grid_for(nb)), dim3(256), 0, p->stream,
                     p->d_bds, nb, p->d_ucblob, p->d_cblob,
                     p->d_ebsize, p->d_ebtype, o.checksum_type, p->d_crc,
                     p->d_ecsum);
  p->kend();
  // per-block boundary keys + seq stats, prefetched with the sizes so the
  // host needs no further GPU round trip for them
  HIPCHK(p->d_scratch_keys.reserve((uint64_t)nb * BLKSTAT_STRIDE));
  HIPCHK(p->h_keys.reserve((uint64_t)nb * BLKSTAT_STRIDE));
  hipLaunchKernelGGL(k_block_stats, dim3(grid_for(nb)), dim3(256), 0, p->stream,
                     p->d_bds, 0u, nb, p->d_sk0, p->d_sk1, p->d_stag,
                     p->d_sklen,
                     general_keys ? p->d_kext.get() : nullptr,
                     p->d_sw, p->d_scratch_keys);
  comp_sizes->resize(nb);
  HIPCHK(hipMemcpyAsync(comp_sizes->data(), p->d_ebsize, sizeof(uint32_t) * nb,
                        hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipMemcpyAsync(p->h_keys.get(), p->d_scratch_keys,
                        (uint64_t)nb * BLKSTAT_STRIDE, hipMemcpyDeviceToHost,
                        p->stream));
  // an emit/compress error would otherwise be silently checksummed and
  // written out as a corrupt block with status OK
  return p->check_err("block emit/compress", err, nullptr, &t);
}

int GpuJob::pack_into(size_t b0, size_t b1, const std::vector<uint64_t>& outoff,
                      uint8_t* host_dst, size_t total_bytes, void** done_event,
                      std::string* err) {
  Impl* p = p_;
  uint32_t nb = (uint32_t)(b1 - b0);
  if (nb == 0) {
    *done_event = nullptr;
    return 0;
  }
  HIPCHK(p->d_outoff.reserve(sizeof(uint64_t) * nb));
  uint64_t* d_outoff = p->d_outoff;
  // synchronous copy: NULL-stream ordering with the (blocking) pipeline
  // stream, no pageable-async lifetime/ordering hazards
  HIPCHK(p->h2d_meta(d_outoff, outoff.data(), sizeof(uint64_t) * nb));
  Impl::OutSlot& slot = p->outslots[p->cur_outslot];
  p->cur_outslot ^= 1;
  if (slot.pending) { // slot reused two files later; transfer long done
    HIPCHK(hipEventSynchronize(slot.done));
    ms_d2h += ms_between(slot.t0, slot.done);
    slot.pending = false;
  }
  HIPCHK(slot.img.reserve(total_bytes));
  p->kbegin("pack", 2.0 * (double)total_bytes);
  hipLaunchKernelGGL(k_pack, dim3(grid_for(nb * 4ull)), dim3(256), 0, p->stream,
                     p->d_bds, (uint32_t)b0, (uint32_t)b1, p->d_ucblob, p->d_cblob,
                     p->d_ebsize, p->d_ebtype, p->d_ecsum,
                     d_outoff, slot.img);
  p->kend();
  // D2H on the copy stream, ordered after the pack kernel via an event; the
  // main stream is free for the next file's kernels immediately
  Event packed;
  (void)hipEventRecord(packed, p->stream);
  HIPCHK(hipStreamWaitEvent(p->d2h_stream, packed, 0));
  (void)hipEventRecord(slot.t0, p->d2h_stream);
  HIPCHK(hipMemcpyAsync(host_dst, slot.img, total_bytes, hipMemcpyDeviceToHost,
                        p->d2h_stream));
  (void)hipEventRecord(slot.done, p->d2h_stream);
  slot.pending = true;
  *done_event = (void*)slot.done.e;
  return 0;
}

int GpuJob::fetch_block_keys(size_t b0, size_t b1,
                             std::vector<std::string>* first_keys,
                             std::vector<std::string>* last_keys,
                             std::string* err) {
  // served from the block-stats records prefetched by emit_blocks (same
  // chunk); no GPU round trip
  Impl* p = p_;
  first_keys->clear();
  last_keys->clear();
  if (b1 <= b0) return 0;
  if (!p->h_keys.get() || b1 > p->emit_nblocks) {
    if (err) *err = "fetch_block_keys: no prefetched chunk stats";
    return -1;
  }
  for (size_t i = b0; i < b1; i++) {
    const uint8_t* o = (const uint8_t*)p->h_keys.get() + i * BLKSTAT_STRIDE;
    first_keys->emplace_back((const char*)o + 1, o[0]);
    last_keys->emplace_back((const char*)o + 65, o[64]);
  }
  return 0;
}

const uint8_t* GpuJob::chunk_stats() const {
  static_assert(GpuJob::kBlkStatStride == BLKSTAT_STRIDE, "stride mismatch");
  return (const uint8_t*)p_->h_keys.get();
}

void GpuJob::block_stats(size_t b, uint64_t* mn, uint64_t* mx, uint64_t* tomb) {
  const uint8_t* o = (const uint8_t*)p_->h_keys.get() + b * BLKSTAT_STRIDE;
  memcpy(mn, o + 128, 8);
  memcpy(mx, o + 136, 8);
  memcpy(tomb, o + 144, 8);
}

int GpuJob::gather_entries(uint64_t first, uint32_t count,
                           std::vector<std::pair<std::string, std::string>>* kvs,
                           std::string* err) {
  Impl* p = p_;
  kvs->clear();
  if (!count) return 0;
  // record layout: [klen u8][key][vlen u32][value]
  std::vector<uint64_t> recoff(count);
  uint64_t acc = 0;
  for (uint32_t i = 0; i < count; i++) {
    recoff[i] = acc;
    acc += 1 + h_klen_[first + i] + 4 + h_vlen_[first + i];
  }
  HIPCHK(p->d_scratch_recoff.reserve(sizeof(uint64_t) * count));
  HIPCHK(p->d_scratch_gather.reserve(acc));
  uint64_t* d_recoff = p->d_scratch_recoff;
  uint8_t* d_out = p->d_scratch_gather;
  HIPCHK(p->h2d_meta(d_recoff, recoff.data(), sizeof(uint64_t) * count));
  hipLaunchKernelGGL(k_gather_range, dim3(grid_for(count)), dim3(256), 0,
                     p->stream, p->d_sk0, p->d_sk1, p->d_stag, p->d_svoff,
                     p->d_svlen, p->d_sklen, p->d_ublob, first, count, d_recoff,
                     general_keys ? p->d_kext.get() : nullptr,
                     p->d_sw, d_out);
  std::vector<uint8_t> h(acc);
  HIPCHK(hipMemcpyAsync(h.data(), d_out, acc, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  for (uint32_t i = 0; i < count; i++) {
    const uint8_t* r = h.data() + recoff[i];
    uint32_t klen = r[0];
    uint32_t vl;
    memcpy(&vl, r + 1 + klen, 4);
    kvs->emplace_back(std::string((const char*)r + 1, klen),
                      std::string((const char*)r + 5 + klen, vl));
  }
  return 0;
}

int GpuJob::gp_positions(const dcw_job_desc* d, std::vector<uint32_t>* pos,
                         std::vector<uint8_t>* nback, std::string* err) {
  Impl* p = p_;
  uint32_t ng = d->num_grandparents;
  uint64_t n = p->n_surv;
  pos->resize(n);
  nback->resize(n);
  if (ng == 0 || n == 0) return 0;
  std::vector<uint64_t> sm0(ng), sm1(ng), lg0(ng), lg1(ng);
  std::vector<uint32_t> smlen(ng), lglen(ng);
  std::vector<uint8_t> tie(ng, 0);
  if (general_keys) { // the worker refuses this before it gets here
    if (err) *err = "grandparent cutting with general-shape keys";
    return -1;
  }
  // a grandparent level may hold keys of any length: the 16-byte padded
  // words plus the true length give raw bytewise order against the job's
  // uniform <= 16 B keys (bound_cmp)
  for (uint32_t g = 0; g < ng; g++) {
    const dcw_grandparent& f = d->grandparents[g];
    uint64_t c;
    make_normkey(f.smallest_ukey, f.smallest_len, 0, &sm0[g], &sm1[g], &c);
    make_normkey(f.largest_ukey, f.largest_len, 0, &lg0[g], &lg1[g], &c);
    smlen[g] = f.smallest_len;
    lglen[g] = f.largest_len;
  }
  // smallest_{g+1} == largest_g on the raw bytes (compaction_outputs.cc:
  // 157-166), not on the padded words
  for (uint32_t g = 0; g + 1 < ng; g++) {
    const dcw_grandparent& f = d->grandparents[g];
    const dcw_grandparent& nx = d->grandparents[g + 1];
    tie[g] = (f.largest_len == nx.smallest_len &&
              memcmp(f.largest_ukey, nx.smallest_ukey, f.largest_len) == 0)
                 ? 1
                 : 0;
  }
  HIPCHK(p->d_gp_sm0.reserve(ng * 8));
  HIPCHK(p->d_gp_sm1.reserve(ng * 8));
  HIPCHK(p->d_gp_lg0.reserve(ng * 8));
  HIPCHK(p->d_gp_lg1.reserve(ng * 8));
  HIPCHK(p->d_gp_smlen.reserve(ng * 4));
  HIPCHK(p->d_gp_lglen.reserve(ng * 4));
  HIPCHK(p->d_gp_tie.reserve(ng));
  HIPCHK(p->d_gp_pos.reserve(n * 4));
  HIPCHK(p->d_gp_nback.reserve(n));
  HIPCHK(p->h2d_meta(p->d_gp_sm0, sm0.data(), ng * 8));
  HIPCHK(p->h2d_meta(p->d_gp_sm1, sm1.data(), ng * 8));
  HIPCHK(p->h2d_meta(p->d_gp_lg0, lg0.data(), ng * 8));
  HIPCHK(p->h2d_meta(p->d_gp_lg1, lg1.data(), ng * 8));
  HIPCHK(p->h2d_meta(p->d_gp_smlen, smlen.data(), ng * 4));
  HIPCHK(p->h2d_meta(p->d_gp_lglen, lglen.data(), ng * 4));
  HIPCHK(p->h2d_meta(p->d_gp_tie, tie.data(), ng));
  hipLaunchKernelGGL(k_gp_positions, dim3(grid_for(n)), dim3(256), 0, p->stream,
                     p->d_sk0, p->d_sk1, n, ukey_len, p->d_gp_sm0,
                     p->d_gp_sm1, p->d_gp_smlen, p->d_gp_lg0,
                     p->d_gp_lg1, p->d_gp_lglen, p->d_gp_tie,
                     ng, p->d_gp_pos, p->d_gp_nback);
  HIPCHK(hipMemcpyAsync(pos->data(), p->d_gp_pos, n * 4, hipMemcpyDeviceToHost,
                        p->stream));
  HIPCHK(hipMemcpyAsync(nback->data(), p->d_gp_nback, n, hipMemcpyDeviceToHost,
                        p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  return 0;
}

int GpuJob::seq_minmax(uint64_t first, uint64_t count, uint64_t* mn, uint64_t* mx,
                       uint64_t* n_tombstones, std::string* err) {
  Impl* p = p_;
  HIPCHK(p->d_scratch_mm.reserve(24));
  unsigned long long* d = p->d_scratch_mm;
  unsigned long long init[3] = {~0ull, 0, 0};
  HIPCHK(p->h2d_meta(d, init, 24));
  hipLaunchKernelGGL(k_seq_minmax, dim3(grid_for(count)), dim3(256), 0, p->stream,
                     p->d_stag, first, count, d, d + 1, d + 2);
  unsigned long long out[3];
  HIPCHK(hipMemcpyAsync(out, d, 24, hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  *mn = out[0];
  *mx = out[1];
  *n_tombstones = out[2];
  return 0;
}

int GpuJob::filter_build(uint64_t first, uint64_t count, uint32_t millibits,
                         std::string* content, uint64_t* n_added,
                         std::string* err) {
  Impl* p = p_;
  HIPCHK(p->d_fhash.reserve(count * 8));
  p->kbegin("filter_hashes", 32.0 * count);
  hipLaunchKernelGGL(k_filter_hashes, dim3(grid_for(count)), dim3(256), 0,
                     p->stream, p->d_sk0, p->d_sk1, p->d_sklen,
                     general_keys ? p->d_kext.get() : nullptr,
                     p->d_sw, first, count,
                     p->d_fhash);
  p->kend();
  // host counts the deduped entries (the filter length depends on it)
  std::vector<uint64_t> h(count);
  HIPCHK(hipMemcpyAsync(h.data(), p->d_fhash, count * 8,
                        hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  uint64_t n = 0;
  for (uint64_t i = 0; i < count; i++)
    if (i == 0 || h[i] != h[i - 1]) n++;
  *n_added = n;
  if (n == 0) {
    content->clear();
    return 0;
  }
  uint64_t lwm = bloom_len_with_metadata(n, millibits);
  uint32_t len = (uint32_t)(lwm - 5);
  int probes = bloom_num_probes((int)millibits);
  HIPCHK(p->d_filter.reserve(lwm + 8));
  HIPCHK(hipMemsetAsync(p->d_filter, 0, lwm + 8, p->stream));
  p->kbegin("filter_bits", 8.0 * count + len);
  hipLaunchKernelGGL(k_filter_bits, dim3(grid_for(count)), dim3(256), 0,
                     p->stream, p->d_fhash, count, len,
                     probes, p->d_filter);
  p->kend();
  content->resize(lwm);
  HIPCHK(hipMemcpyAsync(&(*content)[0], p->d_filter, lwm,
                        hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  p->kresolve();
  // metadata bytes (filter_policy.cc:378-385)
  (*content)[len] = (char)(int8_t)-1;
  (*content)[len + 1] = 0;
  (*content)[len + 2] = (char)probes;
  (*content)[len + 3] = 0;
  (*content)[len + 4] = 0;
  return 0;
}

int GpuJob::dzt_sample(const std::vector<uint32_t>& idx, uint8_t* out,
                       std::string* err) {
  Impl* p = p_;
  uint32_t n = (uint32_t)idx.size();
  if (!n) return 0;
  HIPCHK(p->d_dzt_idx.reserve(n * 4));
  HIPCHK(p->d_dzt_sample.reserve((uint64_t)n * 256));
  HIPCHK(p->h2d_meta(p->d_dzt_idx, idx.data(), n * 4));
  hipLaunchKernelGGL(k_dzt_sample, dim3(grid_for(n)), dim3(256), 0, p->stream,
                     p->d_dzt_idx, n, p->d_svoff, p->d_svlen,
                     p->d_ublob, p->d_dzt_sample);
  HIPCHK(hipMemcpyAsync(out, p->d_dzt_sample, (uint64_t)n * 256,
                        hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  return 0;
}

int GpuJob::dzt_values(const std::vector<DztVBlock>& vbs,
                       const std::vector<uint32_t>& voff_entry,
                       uint64_t ent_base, const uint8_t* dict,
                       uint32_t dict_size, const TableOpts& o,
                       std::vector<uint32_t>* csize, std::vector<uint8_t>* btype,
                       std::vector<uint32_t>* csum, std::string* err) {
  Impl* p = p_;
  uint32_t nvb = (uint32_t)vbs.size();
  if (!nvb) {
    csize->clear();
    btype->clear();
    csum->clear();
    return 0;
  }
  uint64_t stage_total = vbs.back().stage_off + vbs.back().ulen;
  HIPCHK(p->d_dzt_vbs.reserve(sizeof(DztVBlock) * nvb));
  HIPCHK(p->d_dzt_voff.reserve(voff_entry.size() * 4));
  HIPCHK(p->d_dzt_vstage.reserve(stage_total));
  HIPCHK(p->h2d_meta(p->d_dzt_vbs, vbs.data(), sizeof(DztVBlock) * nvb));
  HIPCHK(p->h2d_meta(p->d_dzt_voff, voff_entry.data(), voff_entry.size() * 4));
  p->kbegin("dzt_gather", 2.0 * (double)stage_total);
  hipLaunchKernelGGL(k_dzt_gather, dim3(grid_for(nvb * 64ull)), dim3(256), 0,
                     p->stream, p->d_dzt_vbs, nvb,
                     p->d_dzt_voff, ent_base, p->d_svoff,
                     p->d_svlen, p->d_ublob, p->d_dzt_vstage);
  p->kend();
  // worst-case dict encode is ~1.4x the block (5-byte copy form), larger
  // than snappy_max_compressed's 32+n+n/6 bound for plain snappy
  p->dzt_ccap =
      ((uint64_t)SNAP_MAX_UNC + SNAP_MAX_UNC / 2 + 128 + 63) & ~(uint64_t)63;
  HIPCHK(p->d_dzt_bsize.reserve(nvb * 4));
  HIPCHK(p->d_dzt_btype.reserve(nvb));
  HIPCHK(p->d_dzt_csum.reserve(nvb * 4));
  if (o.compression != 0) {
    HIPCHK(p->d_dzt_dict.reserve(dict_size ? dict_size : 1));
    HIPCHK(p->d_dzt_dict_tab.reserve(sizeof(uint32_t) << kSnapHashBits));
    if (dict_size)
      HIPCHK(p->h2d_meta(p->d_dzt_dict, dict, dict_size));
    HIPCHK(hipMemsetAsync(p->d_dzt_dict_tab, 0xff,
                          sizeof(uint32_t) << kSnapHashBits, p->stream));
    if (dict_size >= 4)
      hipLaunchKernelGGL(k_dict_tab, dim3(grid_for(dict_size)), dim3(256), 0,
                         p->stream, p->d_dzt_dict, dict_size,
                         p->d_dzt_dict_tab);
    HIPCHK(p->d_dzt_cblob.reserve(p->dzt_ccap * nvb));
    p->kbegin("dzt_compress", 1.6 * (double)stage_total);
    uint32_t cgrid = (nvb + 3) / 4;
    hipLaunchKernelGGL(k_dzt_compress, dim3(cgrid < 4096 ? cgrid : 4096),
                       dim3(256), 0, p->stream, p->d_dzt_vbs,
                       nvb, p->d_dzt_vstage,
                       p->d_dzt_dict, dict_size,
                       p->d_dzt_dict_tab,
                       p->d_dzt_cblob, p->dzt_ccap,
                       p->d_dzt_bsize, p->d_dzt_btype,
                       p->d_err);
    p->kend();
  } else {
    // raw blocks: bsize = ulen, btype = 0 (host fills, tiny)
    std::vector<uint32_t> bs(nvb);
    std::vector<uint8_t> bt(nvb, 0);
    for (uint32_t b = 0; b < nvb; b++) bs[b] = vbs[b].ulen;
    HIPCHK(p->h2d_meta(p->d_dzt_bsize, bs.data(), nvb * 4));
    HIPCHK(p->h2d_meta(p->d_dzt_btype, bt.data(), nvb));
    HIPCHK(p->d_dzt_cblob.reserve(64)); // unused
  }
  p->kbegin("dzt_checksum", (double)stage_total);
  hipLaunchKernelGGL(k_dzt_checksum, dim3(grid_for(nvb)), dim3(256), 0,
                     p->stream, p->d_dzt_vbs, nvb,
                     p->d_dzt_vstage,
                     p->d_dzt_cblob, p->dzt_ccap,
                     p->d_dzt_bsize,
                     p->d_dzt_btype, o.checksum_type, p->d_crc,
                     p->d_dzt_csum);
  p->kend();
  csize->resize(nvb);
  btype->resize(nvb);
  csum->resize(nvb);
  HIPCHK(hipMemcpyAsync(csize->data(), p->d_dzt_bsize, nvb * 4,
                        hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipMemcpyAsync(btype->data(), p->d_dzt_btype, nvb,
                        hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipMemcpyAsync(csum->data(), p->d_dzt_csum, nvb * 4,
                        hipMemcpyDeviceToHost, p->stream));
  int rc = p->check_err("DZT value compress", err);
  p->kresolve();
  return rc;
}

int GpuJob::dzt_pack_values(const std::vector<DztVBlock>& vbs,
                            const std::vector<uint64_t>& outoff,
                            uint64_t total_bytes, uint8_t* host_dst,
                            std::string* err) {
  Impl* p = p_;
  uint32_t nvb = (uint32_t)vbs.size();
  if (!nvb) return 0;
  HIPCHK(p->d_outoff.reserve(sizeof(uint64_t) * nvb));
  HIPCHK(p->h2d_meta(p->d_outoff, outoff.data(), sizeof(uint64_t) * nvb));
  HIPCHK(p->d_dzt_img.reserve(total_bytes));
  p->kbegin("dzt_pack", 2.0 * (double)total_bytes);
  hipLaunchKernelGGL(k_dzt_pack, dim3(grid_for(nvb * 4ull)), dim3(256), 0,
                     p->stream, p->d_dzt_vbs, nvb,
                     p->d_dzt_vstage,
                     p->d_dzt_cblob, p->dzt_ccap,
                     p->d_dzt_bsize,
                     p->d_dzt_btype,
                     p->d_dzt_csum,
                     p->d_outoff, p->d_dzt_img);
  p->kend();
  HIPCHK(hipMemcpyAsync(host_dst, p->d_dzt_img, total_bytes,
                        hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipStreamSynchronize(p->stream));
  p->kresolve();
  return 0;
}

int GpuJob::dzt_keyarea(const std::vector<DztKBlock>& kbs,
                        const std::vector<uint32_t>& voff_entry,
                        uint64_t ent_base, uint64_t key_area_size, uint32_t U,
                        uint8_t* host_keyarea, uint8_t* host_first_ikeys,
                        std::string* err) {
  Impl* p = p_;
  uint32_t nkb = (uint32_t)kbs.size();
  if (!nkb) return 0;
  if (U < 1 || U > (general_keys ? (uint32_t)DCW_GKEY_MAX : 16u) ||
      (!general_keys && U != ukey_len)) {
    if (err) *err = "DZT key emit: user-key length outside envelope";
    return -1;
  }
  uint32_t ik = U + 8;
  HIPCHK(p->d_dzt_kbs.reserve(sizeof(DztKBlock) * nkb));
  HIPCHK(p->d_dzt_keyarea.reserve(key_area_size));
  HIPCHK(p->d_dzt_kidx.reserve((uint64_t)nkb * ik));
  HIPCHK(p->h2d_meta(p->d_dzt_kbs, kbs.data(), sizeof(DztKBlock) * nkb));
  // voff_entry already resident from dzt_values (same file)
  (void)voff_entry;
  if (general_keys) {
    // a record moves its key bytes plus tag, not the fast path's 24
    p->kbegin("dzt_keys", (double)ik * (double)nkb * DZTK);
    hipLaunchKernelGGL(k_dzt_keys_g, dim3(grid_for(nkb * 64ull)), dim3(WAVE), 0,
                       p->stream, p->d_dzt_kbs, nkb, p->d_kext.get(), p->d_sw,
                       p->d_stag, p->d_sshared, p->d_dzt_voff, ent_base,
                       p->d_svlen, U, p->d_dzt_keyarea, p->d_dzt_kidx, ik,
                       p->d_err);
  } else {
    p->kbegin("dzt_keys", 24.0 * (double)nkb * DZTK);
    hipLaunchKernelGGL(k_dzt_keys, dim3(grid_for(nkb * 64ull)), dim3(64), 0,
                       p->stream, p->d_dzt_kbs, nkb, p->d_sk0,
                       p->d_sk1, p->d_stag, p->d_sklen, p->d_sshared,
                       p->d_dzt_voff, ent_base, p->d_svlen,
                       ukey_len, p->d_dzt_keyarea,
                       p->d_dzt_kidx, ik, p->d_err);
  }
  p->kend();
  HIPCHK(hipMemcpyAsync(host_keyarea, p->d_dzt_keyarea, key_area_size,
                        hipMemcpyDeviceToHost, p->stream));
  HIPCHK(hipMemcpyAsync(host_first_ikeys, p->d_dzt_kidx, (uint64_t)nkb * ik,
                        hipMemcpyDeviceToHost, p->stream));
  int rc = p->check_err("DZT key emit", err);
  p->kresolve();
  return rc;
}

} // namespace dcw

// ------------------------------------------------------------------
// kernel stats ABI (per-process cumulative; bench.py roofline input)
// ------------------------------------------------------------------
extern "C" int32_t dcw_kernel_stats_json(char* buf, uint32_t cap) {
  std::lock_guard<std::mutex> lk(dcw::g_kmu);
  std::string s = "{";
  bool first = true;
  for (auto& kv : dcw::kstats()) {
    char line[256];
    snprintf(line, sizeof(line),
             "%s\"%s\": {\"launches\": %llu, \"ms\": %.6f, \"alg_bytes\": %.0f}",
             first ? "" : ", ", kv.first.c_str(),
             (unsigned long long)kv.second.launches, kv.second.ms,
             kv.second.alg_bytes);
    s += line;
    first = false;
  }
  s += "}";
  if (s.size() + 1 > cap) return -1;
  memcpy(buf, s.c_str(), s.size() + 1);
  return (int32_t)s.size();
}
extern "C" void dcw_kernel_stats_reset(void) {
  std::lock_guard<std::mutex> lk(dcw::g_kmu);
  dcw::kstats().clear();
}
