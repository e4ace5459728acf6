// dcw_zstd_dict.h — preset dictionaries for the zstd frame decoders of
// dcw_zstd_dec.h and dcw_zstd_dec_large.h.  Included by dcw_dict.hip for the
// GPU (k_zstd_dict_prepare, k_decompress_zstd_dict,
// k_decompress_zstd_large_dict) and by tools/zstd_dict_host.
//
// A BlockBasedTable file whose blocks were coded against a dictionary carries
// it, uncompressed, as the meta block "rocksdb.compression_dict"
// (block_based_table_builder.cc:1712-1733, written by Finish() at :1960); the
// reader hands it to every block's decoder (util/compression.h:1390-1424,
// ZSTD_decompress_usingDDict / ZSTD_decompress_usingDict).  libzstd takes it
// in one of two forms (ZSTD_decompress_insertDictionary):
//   full   magic 0xEC30A437, Dictionary_ID, a Huffman tree description, FSE
//          table descriptions for offsets, match lengths and literal lengths
//          in that order, three 4-byte repeat offsets, then the content.  A
//          frame then starts with these tables and offsets in place, so its
//          first block may have treeless literals and Repeat_Mode tables.
//   raw    anything else: the whole block is content, Dictionary_ID 0.
// Either way the content is a prefix of every frame's output: an offset may
// reach back past output byte 0 into the content's tail.
//
// zstd_dict_prepare() turns one dictionary into a ZstdDictTables record, once
// per job, with the table builders of dcw_zstd_dec.h.  The decoders take the
// record and the content through the policies ZMemLdsDict / ZMemGlobalDict:
// the record's tables are copied into the wave's state behind each frame
// header, 16 bytes per lane per step; the content stays where the file was
// staged and is read by the matches that reach it.
#pragma once
#include "dcw_zstd_dec_large.h"

namespace dcw {

static const uint32_t kZstdDictMagic = 0xEC30A437u;

// What a dictionary's blocks need of it, in global memory.  tLL..huf are in
// the layout of the wave states, each a multiple of 16 bytes.
struct alignas(16) ZstdDictTables {
  uint64_t tLL[512], tML[512], tOF[256];
  uint16_t huf[2048];
  uint32_t hlog, tlog[3];
  uint32_t rep[3], dict_id;
  uint32_t full;        // tables and repeat offsets are valid
  uint32_t content_off; // content = dictionary[content_off, +content_len)
  uint32_t content_len;
  uint32_t fail;        // a full dictionary that libzstd refuses: no block decodes
};

#if defined(__HIPCC__)
// One entry of a job's dictionary table: where the dictionary lies in the
// staged blob, and its ZstdDictTables record (0xffffffff: none, no zstd block
// uses it).  dcw_dict.hip has the kernels behind the launchers.
struct DictDev {
  uint64_t off;
  uint32_t size, tab;
};
static const uint32_t kNoDict = 0xffffffffu; // a block's slot: no dictionary
void launch_zstd_dict_prepare(hipStream_t stream, const uint8_t* blob,
                              const DictDev* dicts, uint32_t ndicts,
                              ZstdDictTables* tabs);
// the three decode launchers take the block tables of k_decompress_lz4 plus
// `slot`, parallel to `list`: each block's entry of `dicts` or kNoDict
struct DictDecodeArgs {
  const uint8_t* blob;
  const uint64_t* boff;
  const uint32_t* bsize;
  const uint64_t* uoff;
  const uint32_t* usize;
  const uint32_t* list;
  const uint32_t* slot;
  uint32_t nlist;
  const DictDev* dicts;
  const ZstdDictTables* tabs;
  uint8_t* ublob;
  uint32_t* err_flag;
  uint32_t err_code;
};
void launch_decompress_zstd_dict(uint32_t grid, hipStream_t stream,
                                 const DictDecodeArgs& a);
void launch_decompress_zstd_large_dict(uint32_t grid, hipStream_t stream,
                                       const DictDecodeArgs& a, uint8_t* litscr);
void launch_decompress_lz4_dict(uint32_t grid, hipStream_t stream,
                                const DictDecodeArgs& a);
#endif

#ifdef DCW_ZSTD_WAVE
// ---- the dictionary beside a memory policy.  T == nullptr: no dictionary,
// the frame decodes as under the plain policy.
struct ZDict {
  const ZstdDictTables* T;
  const uint8_t* end; // one past the content
  uint32_t len;       // content bytes
};
ZFN ZDict z_dict(const ZstdDictTables* T, const uint8_t* dict) {
  ZDict d = {T, nullptr, 0};
  if (T) {
    d.end = dict + T->content_off + T->content_len;
    d.len = T->content_len;
  }
  return d;
}
struct ZMemLdsDict : ZMemLds { ZDict d; };
struct ZMemGlobalDict : ZMemGlobal { ZDict d; };

ZFN bool zm_has_dict(const ZMemLdsDict& m) { return m.d.T != nullptr; }
ZFN bool zm_has_dict(const ZMemGlobalDict& m) { return m.d.T != nullptr; }
ZFN uint32_t zm_dict_id(const ZMemLdsDict& m) { return m.d.T->dict_id; }
ZFN uint32_t zm_dict_id(const ZMemGlobalDict& m) { return m.d.T->dict_id; }
ZFN uint32_t zm_prefix_len(const ZMemLdsDict& m) { return m.d.len; }
ZFN uint32_t zm_prefix_len(const ZMemGlobalDict& m) { return m.d.len; }

// Behind the frame header: a full dictionary's tables and repeat offsets into
// the state (~14 KiB; 16 bytes per lane per step).  The frame then starts as
// libzstd's does after ZSTD_loadDEntropy: litEntropy = fseEntropy = 1.
template <class ZS>
ZFN void z_dict_frame_begin(ZS& S, const ZDict& d, uint32_t zlane) {
  (void)zlane;
  if (!d.T || !d.T->full) return;
  const ZstdDictTables* T = d.T;
  const uint8_t* src = (const uint8_t*)T->tLL;
  uint8_t* dst = (uint8_t*)S.tLL; // tLL, tML, tOF are one stretch in both
  const uint32_t nfse = (512 + 512 + 256) * 8, nhuf = 2048 * 2;
  ZL_COPY(dst, src, nfse)
  src = (const uint8_t*)T->huf;
  dst = (uint8_t*)S.huf;
  ZL_COPY(dst, src, nhuf)
  ZW_LANES {
    if (lane != 0) continue;
    S.have_huf = S.have_fse = 1;
    S.hlog = T->hlog;
    for (uint32_t t = 0; t < 3; t++) {
      S.tlog[t] = T->tlog[t];
      S.tpre[t] = 0;
    }
    S.rep1 = T->rep[0]; S.rep2 = T->rep[1]; S.rep3 = T->rep[2];
  }
  ZW_SYNC();
}
ZFN void zm_frame_begin(ZstdWave& S, const ZMemLdsDict& m, uint32_t zlane) {
  z_dict_frame_begin(S, m.d, zlane);
}
ZFN void zm_frame_begin(ZstdLargeLds& S, const ZMemGlobalDict& m, uint32_t zlane) {
  z_dict_frame_begin(S, m.d, zlane);
}

// A match of ml bytes to d = output + at whose source starts before output
// byte 0 (off > at; off <= at + len was checked): its first off - at bytes,
// or all of it, come from the content's tail.  -> bytes moved; what is left
// is the usual move at the same offset, whose source is now output byte 0.
ZFN uint32_t z_dict_part(const ZDict& dc, uint8_t* d, uint32_t at, uint32_t off,
                         uint32_t ml, uint32_t zlane) {
  (void)zlane;
  if (off <= at) return 0;
  const uint32_t need = off - at, c = need < ml ? need : ml;
  const uint8_t* s = dc.end - need;
  ZW_LANES { for (uint32_t i = lane; i < c; i += 64) d[i] = s[i]; }
  ZW_SYNC();
  return c;
}
ZFN uint32_t zm_dict_part(const ZMemLdsDict& m, uint8_t* d, uint32_t at, uint32_t off,
                          uint32_t ml, uint32_t zlane) {
  return z_dict_part(m.d, d, at, off, ml, zlane);
}
ZFN uint32_t zm_dict_part(const ZMemGlobalDict& m, uint8_t* d, uint32_t at,
                          uint32_t off, uint32_t ml, uint32_t zlane) {
  return z_dict_part(m.d, d, at, off, ml, zlane);
}

// The frame in S.in[0, n) -> S.out[0, cap) with dictionary `dict` prepared as
// T (both nullptr: none).  A dictionary whose record says fail refuses.
ZFN bool zstd_dec_wave_dict(ZstdWave& S, const ZstdDictTables* T, const uint8_t* dict,
                            uint32_t n, uint32_t cap, uint32_t zlane) {
  if (T && T->fail) return false;
  ZMemLdsDict m;
  m.d = z_dict(T, dict);
  return zstd_dec_frame(S, m, n, cap, zlane);
}
ZFN bool zstd_dec_wave_large_dict(ZstdLargeLds& S, const ZMemGlobal& g,
                                  const ZstdDictTables* T, const uint8_t* dict,
                                  uint32_t n, uint32_t cap, uint32_t zlane) {
  if (T && T->fail) return false;
  ZMemGlobalDict m;
  m.in = g.in; m.out = g.out; m.lit = g.lit;
  m.d = z_dict(T, dict);
  return zstd_dec_frame(S, m, n, cap, zlane);
}

// ---- dictionary[0, n) -> *T by one wave, S its scratch state.  Every
// decision is taken on S; *T is stored at the end, whole, or for a refused
// dictionary its fail flag alone.  The bounds are libzstd's
// (ZSTD_loadDEntropy): each description inside the dictionary, table logs at
// most 8 / 9 / 9, 12 bytes of repeat offsets, each of them 1..content length;
// the Huffman table log at most 11 as everywhere in this decoder.
ZFN void zstd_dict_prepare(ZstdLargeLds& S, const uint8_t* dict, uint32_t n,
                           ZstdDictTables* T, uint32_t zlane) {
  uint32_t magic = 0;
  if (n >= 8) memcpy(&magic, dict, 4);
  if (magic != kZstdDictMagic) { // raw content (libzstd: also under 8 bytes)
    ZW_LANES {
      if (lane != 0) continue;
      T->full = 0; T->fail = 0; T->dict_id = 0;
      T->content_off = 0; T->content_len = n;
    }
    ZW_SYNC();
    return;
  }
  ZW_LANES {
    if (lane != 0) continue;
    S.fail = 0;
    S.need_wfse = 0;
    S.ip = zstd_huf_tree_desc(S, dict, 8, n - 8);
    if (S.ip == 0) S.fail = 1;
    S.ip += 8;
  }
  ZW_SYNC();
  if (!S.fail && S.need_wfse) {
    zstd_fse_build(S, S.tW, ZT_W, zlane);
    ZW_LANES { if (lane == 0) zstd_huf_fse_weights(S, dict); }
    ZW_SYNC();
  }
  if (!S.fail) zstd_huf_build(S, zlane);
  for (uint32_t k = 0; k < 3 && !S.fail; k++) { // offsets, match lengths, literal lengths
    const uint32_t t = k == 0 ? ZT_OF : k == 1 ? ZT_ML : ZT_LL;
    ZW_LANES {
      if (lane != 0) continue;
      uint32_t c = zstd_read_ncount(S, dict + S.ip, n - S.ip, t == ZT_LL ? 35 : t == ZT_OF ? 31 : 52,
                                    t == ZT_OF ? 8 : 9);
      if (c == 0) S.fail = 1;
      S.ip += c;
      S.tlog[t] = S.blog;
    }
    ZW_SYNC();
    if (!S.fail)
      zstd_fse_build(S, t == ZT_LL ? S.tLL : t == ZT_OF ? S.tOF : S.tML, t, zlane);
  }
  ZW_LANES {
    if (lane != 0 || S.fail) continue;
    if (n - S.ip < 12) { S.fail = 1; continue; }
    const uint32_t clen = n - S.ip - 12;
    uint32_t r[3];
    memcpy(r, dict + S.ip, 12);
    for (uint32_t k = 0; k < 3; k++)
      if (r[k] == 0 || r[k] > clen) S.fail = 1;
    S.rep1 = r[0]; S.rep2 = r[1]; S.rep3 = r[2];
  }
  ZW_SYNC();
  if (S.fail) {
    ZW_LANES { if (lane == 0) T->fail = 1; }
    ZW_SYNC();
    return;
  }
  {
    const uint8_t* src = (const uint8_t*)S.tLL;
    uint8_t* dst = (uint8_t*)T->tLL;
    const uint32_t nfse = (512 + 512 + 256) * 8, nhuf = 2048 * 2;
    ZL_COPY(dst, src, nfse)
    src = (const uint8_t*)S.huf;
    dst = (uint8_t*)T->huf;
    ZL_COPY(dst, src, nhuf)
  }
  ZW_LANES {
    if (lane != 0) continue;
    T->hlog = S.hlog;
    for (uint32_t t = 0; t < 3; t++) T->tlog[t] = S.tlog[t];
    T->rep[0] = S.rep1; T->rep[1] = S.rep2; T->rep[2] = S.rep3;
    memcpy(&T->dict_id, dict + 4, 4);
    T->full = 1; T->fail = 0;
    T->content_off = S.ip + 12;
    T->content_len = n - S.ip - 12;
  }
  ZW_SYNC();
}
#endif // DCW_ZSTD_WAVE

} // namespace dcw
