// dcw_k_merge.h — merge, dedup FSM, scan and survivor-gather kernels.
// A section of the single GPU translation unit: dcw_gpu.hip includes the
// dcw_k_*.h headers in order, inside one unit, so every kernel is defined
// before the host code that launches it.  Not a stand-alone header.
#pragma once
#include "dcw_bound_cmp.h"

namespace dcw {

// ------------------------------------------------------------------
// merge
// ------------------------------------------------------------------
__device__ uint64_t merge_diag(const ulong4* A, uint64_t nA, const ulong4* B,
                               uint64_t nB, uint64_t d,
                               const uint8_t* kext, const uint8_t* klen) {
  // largest a in [max(0,d-nB), min(d,nA)] s.t. A[0..a) all <= B from b=d-a on
  uint64_t lo = d > nB ? d - nB : 0;
  uint64_t hi = d < nA ? d : nA;
  while (lo < hi) {
    uint64_t mid = (lo + hi + 1) / 2;
    // A[mid-1] vs B[d-mid]: A goes first on ties
    if (ent_le_g(A[mid - 1], B[d - mid], kext, klen))
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

template <int ITEMS>
__global__ void k_merge_pair(const ulong4* __restrict__ A, uint64_t nA,
                             const ulong4* __restrict__ B, uint64_t nB,
                             ulong4* __restrict__ out) {
  uint64_t total = nA + nB;
  uint64_t nchunk = (total + ITEMS - 1) / ITEMS;
  for (uint64_t c = blockIdx.x * blockDim.x + threadIdx.x; c < nchunk;
       c += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t d0 = c * ITEMS;
    uint64_t d1 = d0 + ITEMS < total ? d0 + ITEMS : total;
    uint64_t a = merge_diag(A, nA, B, nB, d0, nullptr, nullptr);
    uint64_t b = d0 - a;
    for (uint64_t d = d0; d < d1; d++) {
      bool takeA = a < nA && (b >= nB || ent_le(A[a], B[b]));
      out[d] = takeA ? A[a++] : B[b++];
    }
  }
}

// LDS-tiled merge: each 256-thread workgroup merges one 2048-entry output
// tile.  The A/B segments for the tile are staged into LDS with fully
// coalesced 32 B loads, each thread finds its private diagonal in LDS and
// merges 8 entries, and the tile's output range is contiguous, so stores
// coalesce too.  Removes the ~10x HBM over-fetch of the per-thread global
// merge (profiles/pmc_hbm_traffic_r01.txt).
#define MT_TILE 2048
#define MT_TPB 256
#define MT_ITEMS (MT_TILE / MT_TPB)
__device__ __forceinline__ bool ent_le_s(const ulong4& a, const ulong4& b) {
  if (a.x != b.x) return a.x < b.x;
  if (a.y != b.y) return a.y < b.y;
  return a.z <= b.z;
}
// tile boundaries for k_merge_tiled, one thread per boundary: with ~1
// tile per workgroup the two ~21-step dependent-load binary searches
// would otherwise run serially on thread 0 of every workgroup (255
// threads idle) and dominate the pair-merge latency; here they all
// overlap in one small launch
__global__ void k_merge_diags(const ulong4* __restrict__ A, uint64_t nA,
                              const ulong4* __restrict__ B, uint64_t nB,
                              const uint8_t* __restrict__ kext,
                              const uint8_t* __restrict__ klen,
                              uint64_t ntiles, uint64_t* __restrict__ diags) {
  uint64_t total = nA + nB;
  for (uint64_t t = blockIdx.x * blockDim.x + threadIdx.x; t <= ntiles;
       t += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t d = t * MT_TILE;
    if (d > total) d = total;
    diags[t] = merge_diag(A, nA, B, nB, d, kext, klen);
  }
}
__global__ __launch_bounds__(MT_TPB) void k_merge_tiled(
    const ulong4* __restrict__ A, uint64_t nA, const ulong4* __restrict__ B,
    uint64_t nB, ulong4* __restrict__ out, const uint8_t* __restrict__ kext,
    const uint8_t* __restrict__ klen, const uint64_t* __restrict__ diags) {
  __shared__ ulong4 S[MT_TILE]; // A-segment then B-segment
  __shared__ uint32_t seg[2];   // nA_t, a0 broadcast... [0]=nA_t
  __shared__ uint64_t base[2];  // a0, b0
  uint64_t total = nA + nB;
  uint64_t ntiles = (total + MT_TILE - 1) / MT_TILE;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint64_t d0 = t * MT_TILE;
    uint64_t d1 = d0 + MT_TILE < total ? d0 + MT_TILE : total;
    if (threadIdx.x == 0) {
      uint64_t a0 = diags ? diags[t] : merge_diag(A, nA, B, nB, d0, kext, klen);
      uint64_t a1 =
          diags ? diags[t + 1] : merge_diag(A, nA, B, nB, d1, kext, klen);
      base[0] = a0;
      base[1] = d0 - a0;
      seg[0] = (uint32_t)(a1 - a0);
      seg[1] = (uint32_t)((d1 - a1) - (d0 - a0));
    }
    __syncthreads();
    uint64_t a0 = base[0], b0 = base[1];
    uint32_t na = seg[0], nbt = seg[1];
    for (uint32_t i = threadIdx.x; i < na; i += MT_TPB) S[i] = A[a0 + i];
    for (uint32_t i = threadIdx.x; i < nbt; i += MT_TPB) S[na + i] = B[b0 + i];
    __syncthreads();
    // per-thread diagonal within the LDS tile
    uint32_t tile_n = na + nbt;
    uint32_t td0 = threadIdx.x * MT_ITEMS;
    if (td0 < tile_n) {
      uint32_t td1 = td0 + MT_ITEMS < tile_n ? td0 + MT_ITEMS : tile_n;
      // largest a in [max(0,td0-nbt), min(td0,na)] with S[a-1] <= Bs[td0-a]
      uint32_t lo = td0 > nbt ? td0 - nbt : 0;
      uint32_t hi = td0 < na ? td0 : na;
      while (lo < hi) {
        uint32_t mid = (lo + hi + 1) / 2;
        if (ent_le_g(S[mid - 1], S[na + (td0 - mid)], kext, klen))
          lo = mid;
        else
          hi = mid - 1;
      }
      uint32_t a = lo, b = td0 - lo;
      ulong4 regs[MT_ITEMS];
      for (uint32_t d = td0; d < td1; d++) {
        bool takeA = a < na && (b >= nbt || ent_le_g(S[a], S[na + b], kext, klen));
        regs[d - td0] = takeA ? S[a++] : S[na + b++];
      }
      for (uint32_t d = td0; d < td1; d++) out[d0 + d] = regs[d - td0];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------
// dedup / visibility
// ------------------------------------------------------------------
__global__ void k_mark_heads(const ulong4* __restrict__ e, uint64_t n,
                             const uint8_t* __restrict__ kext,
                             const uint8_t* __restrict__ klen,
                             uint8_t* __restrict__ head) {
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    bool h = (i == 0) || e[i].x != e[i - 1].x || e[i].y != e[i - 1].y;
    if (!h && kext) h = gkey_cmp(kext, klen, e[i].w, e[i - 1].w) != 0;
    head[i] = h;
  }
}

struct FsmParams {
  uint64_t earliest_snapshot;
  uint64_t ewcs;
  const uint64_t* snapshots;
  uint32_t num_snapshots;
  uint32_t visible_at_tip;
  uint32_t bottommost;
  uint32_t levels_below_valid;
  // levels-below normkey ranges, concatenated; per-level [begin,end) offsets
  const uint64_t* lb_sm_k0;
  const uint64_t* lb_sm_k1;
  const uint64_t* lb_lg_k0;
  const uint64_t* lb_lg_k1;
  const uint32_t* lb_level_beg; // num_levels+1
  uint32_t num_levels;
  // true byte length of each boundary: a level below may hold keys of any
  // length, and the padded words alone cannot order "K" against "K\0"
  const uint32_t* lb_sm_len;
  const uint32_t* lb_lg_len;
  // general-key mode only (null otherwise): the first DCW_GKEY_MAX bytes of
  // each boundary at DCW_GKEY_STRIDE, and the job's full-key side table
  const uint8_t* lb_sm_ext;
  const uint8_t* lb_lg_ext;
  const uint8_t* kext;
  const uint8_t* klen;
  // range-deletion fragments (GpuJob::RdFrag SoA; envelope subset)
  const uint64_t* rd_k0;
  const uint64_t* rd_k1;
  const uint32_t* rd_len;
  const uint8_t* rd_ext; // general-key mode only, like lb_sm_ext
  const uint64_t* rd_seq;
  uint32_t num_rd;
  uint32_t rd_ukey_len; // the job's uniform user-key length
};

// covered iff the fragment containing the user key has max_seq > seq
// (range_del_aggregator.cc:407-413 single-stripe rule).  The fragment is
// found in raw bytewise order through bound_cmp (dcw_bound_cmp.h, where the
// argument for the search staying monotone on starts it cannot tell apart
// is written down).  w: payload index of the group's first entry.
__device__ __forceinline__ bool fsm_rd_covers(const FsmParams& P, uint64_t k0,
                                              uint64_t k1, uint64_t w,
                                              uint64_t seq) {
  const uint8_t* kfull = P.kext ? P.kext + w * DCW_GKEY_STRIDE : nullptr;
  uint32_t ulen = P.kext ? (uint32_t)P.klen[w] - 8 : P.rd_ukey_len;
  uint32_t lo = rd_frag_upper(P.rd_k0, P.rd_k1, P.rd_len, P.rd_ext, P.num_rd,
                              k0, k1, ulen, kfull);
  if (lo == 0) return false;
  return P.rd_seq[lo - 1] > seq;
}

__device__ uint64_t fsm_find_earliest(const FsmParams& P, uint64_t seq,
                                      uint64_t* prev) {
  uint32_t lo = 0, hi = P.num_snapshots;
  while (lo < hi) {
    uint32_t mid = (lo + hi) / 2;
    if (P.snapshots[mid] < seq)
      lo = mid + 1;
    else
      hi = mid;
  }
  *prev = lo > 0 ? P.snapshots[lo - 1] : 0;
  return lo < P.num_snapshots ? P.snapshots[lo] : kMaxSeq;
}

// w: payload index of the group's first entry (general mode: its full key)
__device__ bool fsm_key_not_exists_beyond(const FsmParams& P, uint64_t k0,
                                          uint64_t k1, uint64_t w) {
  if (P.bottommost) return true;
  if (!P.levels_below_valid) return false; // reference worker branch
  const uint8_t* kfull = P.kext ? P.kext + w * DCW_GKEY_STRIDE : nullptr;
  uint32_t ulen = P.kext ? (uint32_t)P.klen[w] - 8 : P.rd_ukey_len;
  for (uint32_t lvl = 0; lvl < P.num_levels; lvl++) {
    uint32_t b = P.lb_level_beg[lvl], e = P.lb_level_beg[lvl + 1];
    // first file with largest >= key
    uint32_t lo = b, hi = e;
    while (lo < hi) {
      uint32_t mid = (lo + hi) / 2;
      // compaction.cc:566: Compare(user_key, largest) <= 0 ends the walk
      bool lg_lt =
          bound_cmp(P.lb_lg_k0[mid], P.lb_lg_k1[mid], P.lb_lg_len[mid],
                    kfull ? P.lb_lg_ext + (uint64_t)mid * DCW_GKEY_STRIDE : nullptr,
                    k0, k1, ulen, kfull) < 0;
      if (lg_lt)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < e) {
      // compaction.cc:573-577: Compare(user_key, smallest) >= 0 -> may exist
      bool sm_le =
          bound_cmp(P.lb_sm_k0[lo], P.lb_sm_k1[lo], P.lb_sm_len[lo],
                    kfull ? P.lb_sm_ext + (uint64_t)lo * DCW_GKEY_STRIDE : nullptr,
                    k0, k1, ulen, kfull) <= 0;
      if (sm_le) return false;
    }
  }
  return true;
}

// group flags
enum : uint8_t { GF_PRODUCED = 1, GF_LAG_SENSITIVE = 2 };

// One thread per user-key group.  Mirrors CompactionIterator::NextFromInput
// (:475-1082) + PrepareOutput seq-zeroing (:1286-1328), restricted to one
// user key (all FSM state resets at user-key change, :568-583).
// is_first_group_mode: 0 = normal pass (has_outputted = outputs>=1),
// group `lag_group` (if != ~0) uses outputs>=2 (SeekToFirst lag,
// compaction_iterator.cc:156-159 + 223-226).
__global__ void k_group_fsm(const ulong4* __restrict__ e, uint64_t n,
                            const uint64_t* __restrict__ head_idx,
                            uint64_t ngroups, FsmParams P,
                            uint8_t* __restrict__ survive,
                            uint64_t* __restrict__ newtag,
                            uint8_t* __restrict__ clearv,
                            uint8_t* __restrict__ gflags, uint64_t lag_group,
                            uint32_t* err_flag) {
  for (uint64_t g = blockIdx.x * blockDim.x + threadIdx.x; g < ngroups;
       g += (uint64_t)gridDim.x * blockDim.x) {
    if (lag_group != ~0ull && g != lag_group) continue;
    uint64_t g0 = head_idx[g];
    uint64_t g1 = g + 1 < ngroups ? head_idx[g + 1] : n;
    uint64_t k0 = e[g0].x, k1 = e[g0].y;
    bool is_lag = (g == lag_group);
    int outputs = 0;
    bool clear_next = false, last_zeroed = false, lag_sensitive = false;
    uint64_t cukSnap = 0;
    bool first_entry = true;
    uint64_t pos = g0;
    while (pos < g1) {
      uint64_t tag = ~e[pos].z;
      uint64_t seq = tag >> 8;
      uint8_t type = (uint8_t)tag;
      uint64_t last_snapshot = first_entry ? 0 : cukSnap;
      first_entry = false;
      uint64_t prev_snapshot = 0;
      cukSnap = P.visible_at_tip ? P.earliest_snapshot
                                 : fsm_find_earliest(P, seq, &prev_snapshot);
      survive[pos] = 0;
      clearv[pos] = 0;
      newtag[pos] = tag;
      bool has_outputted = is_lag ? outputs >= 2 : outputs >= 1;
      bool out_this = false, clear_this = false;
      uint64_t consumed = 1;
      if (clear_next) {
        if (type != kTypeValue) {
          set_err(err_flag, DE_TYPE);
          return;
        }
        out_this = true;
        clear_this = true;
        clear_next = false;
      } else if (type == kTypeSingleDeletion) {
        if (outputs == 1) lag_sensitive = true; // decision may depend on lag
        if (pos + 1 < g1) {
          uint64_t ntag = ~e[pos + 1].z;
          uint64_t nseq = ntag >> 8;
          uint8_t ntype = (uint8_t)ntag;
          if (last_zeroed) {
            consumed = 2; // drop SD and the next version
          } else if (prev_snapshot == 0 || nseq > prev_snapshot) {
            if (ntype == kTypeSingleDeletion) {
              consumed = 1; // skip the first SD; reprocess the second
            } else if (ntype == kTypeDeletion) {
              set_err(err_flag, DE_SD_CONTRACT);
              return;
            } else if (has_outputted || seq <= P.ewcs ||
                       (P.earliest_snapshot < P.ewcs &&
                        seq <= P.earliest_snapshot)) {
              consumed = 2; // drop both SD and value
            } else {
              out_this = true; // kKeepSDForConflictCheck
              clear_next = true;
            }
          } else {
            out_this = true; // kKeepSDForSnapshot
          }
        } else {
          if (seq <= P.earliest_snapshot &&
              fsm_key_not_exists_beyond(P, k0, k1, e[g0].w)) {
            // drop (fallthrough SD)
          } else if (last_zeroed) {
            // drop
          } else {
            out_this = true; // kKeepSD
          }
        }
      } else if (last_snapshot == cukSnap ||
                 (last_snapshot > 0 && last_snapshot < cukSnap)) {
        // rule (A): hidden by newer entry in the same snapshot stripe
      } else if (type == kTypeDeletion && seq <= P.earliest_snapshot &&
                 fsm_key_not_exists_beyond(P, k0, k1, e[g0].w)) {
        // obsolete delete
      } else if (type == kTypeDeletion && P.bottommost) {
        // skip versions in the same snapshot range
        uint64_t j = pos + 1;
        while (j < g1) {
          uint64_t jseq = (~e[j].z) >> 8;
          if (!(prev_snapshot == 0 || jseq > prev_snapshot)) break;
          j++;
        }
        if (j < g1) {
          out_this = true; // kKeepDel
          consumed = j - pos;
        } else {
          consumed = g1 - pos; // drop delete and all covered versions
        }
      } else if (P.num_rd && fsm_rd_covers(P, k0, k1, e[g0].w, seq)) {
        // dropped by a range tombstone (compaction_iterator.cc:1056-1063:
        // the ShouldDelete site is the final keep branch only)
      } else {
        out_this = true; // kNewUserKey / plain keep
      }
      if (out_this) {
        uint64_t otag = tag;
        // PrepareOutput seq-zeroing (bottommost, visible in every snapshot)
        if (P.bottommost && seq <= P.earliest_snapshot && type == kTypeValue) {
          otag = (uint64_t)type;
          last_zeroed = true;
        }
        survive[pos] = 1;
        newtag[pos] = otag;
        clearv[pos] = clear_this ? 1 : 0;
        outputs++;
      }
      pos += consumed;
    }
    if (gflags)
      gflags[g] = (outputs > 0 ? GF_PRODUCED : 0) |
                  (lag_sensitive ? GF_LAG_SENSITIVE : 0);
  }
}

// ------------------------------------------------------------------
// scans (u32 exclusive scan, two-level with host combining the block sums)
// ------------------------------------------------------------------
__global__ void k_scan_partial(const uint8_t* __restrict__ in, uint64_t n,
                               uint32_t* __restrict__ out,
                               uint32_t* __restrict__ block_sums) {
  __shared__ uint32_t tmp[1024];
  uint64_t base = (uint64_t)blockIdx.x * 1024;
  uint32_t t = threadIdx.x;
  uint32_t v = (base + t < n) ? in[base + t] : 0;
  tmp[t] = v;
  __syncthreads();
  // Hillis-Steele in LDS
  for (uint32_t off = 1; off < 1024; off *= 2) {
    uint32_t x = (t >= off) ? tmp[t - off] : 0;
    __syncthreads();
    tmp[t] += x;
    __syncthreads();
  }
  if (base + t < n) out[base + t] = tmp[t] - v; // exclusive
  if (t == 1023) block_sums[blockIdx.x] = tmp[t];
}
__global__ void k_scan_add_base(uint32_t* __restrict__ out, uint64_t n,
                                const uint32_t* __restrict__ base_per_block) {
  uint64_t i = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
  if (i < n) out[i] += base_per_block[blockIdx.x];
}

// ------------------------------------------------------------------
// survivor gather + shared-prefix
// ------------------------------------------------------------------
__global__ void k_gather_survivors(
    const ulong4* __restrict__ e, uint64_t n, const uint8_t* __restrict__ survive,
    const uint32_t* __restrict__ pos, const uint64_t* __restrict__ newtag,
    const uint8_t* __restrict__ clearv, const uint64_t* __restrict__ voff,
    const uint32_t* __restrict__ vlen, const uint8_t* __restrict__ klen,
    uint64_t* __restrict__ s_k0, uint64_t* __restrict__ s_k1,
    uint64_t* __restrict__ s_tag, uint64_t* __restrict__ s_voff,
    uint32_t* __restrict__ s_vlen, uint8_t* __restrict__ s_klen,
    uint32_t* __restrict__ s_w) {
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    if (!survive[i]) continue;
    uint32_t o = pos[i];
    uint64_t ref = e[i].w;
    s_k0[o] = e[i].x;
    s_k1[o] = e[i].y;
    s_tag[o] = newtag[i];
    s_voff[o] = voff[ref];
    s_vlen[o] = clearv[i] ? 0 : vlen[ref];
    s_klen[o] = klen[ref];
    s_w[o] = (uint32_t)ref;
  }
}

} // namespace dcw
