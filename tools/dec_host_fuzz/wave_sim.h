// host simulation of snap_dec_wave's batch/round structure (shared by
// wave_fuzz.cpp and corpus_check.cpp)
#pragma once
#include <cstdint>
#include <cstring>
#include <cstdio>
static inline uint64_t ld64(const uint8_t* p){uint64_t v;memcpy(&v,p,8);return v;}
static inline void st64(uint8_t* p,uint64_t v){memcpy(p,&v,8);}
struct Op { uint32_t dst, src, len, kind; };
// mirrors snap_dec_wave: lockstep parse == single parse; rounds as on device
static uint32_t dec_wave_sim(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap) {
  uint32_t ulen = 0, ip = 0;
  { uint64_t h = ld64(in); uint32_t s = 0;
    for (;;) { if (ip >= n || ip >= 5) return 0;
      uint8_t b = (uint8_t)(h >> (8*ip)); ulen |= (uint32_t)(b & 0x7f) << s; ip++;
      if (!(b & 0x80)) break; s += 7; } }
  if (ulen > cap) return 0;
  uint32_t opos = 0;
  while (ip < n) {
    Op ops[64]; uint32_t nops = 0;
    while (ip < n && nops < 64) {
      uint64_t h = ld64(in + ip); uint8_t tag = (uint8_t)h;
      uint32_t len, srcp, kind;
      if ((tag & 3) == 0) {
        len = (uint32_t)(tag >> 2) + 1; uint32_t hb = 1;
        if (len > 60) { uint32_t nb = len - 60;
          if (ip + 1 + nb > n) return 0;
          uint32_t lm1 = (uint32_t)((h >> 8) & (0xffffffffull >> (8*(4-nb))));
          if (lm1 >= n) return 0;
          len = lm1 + 1; hb = 1 + nb; }
        ip += hb;
        if (ip + len > n || opos + len > ulen) return 0;
        srcp = ip; kind = 1; ip += len;
      } else {
        uint32_t offset, hb;
        if ((tag & 3) == 1) { len = ((uint32_t)(tag>>2)&7)+4; offset = ((uint32_t)(tag>>5)<<8)|(uint8_t)(h>>8); hb = 2; }
        else if ((tag & 3) == 2) { len = (uint32_t)(tag>>2)+1; offset = (uint32_t)(h>>8)&0xffffu; hb = 3; }
        else { len = (uint32_t)(tag>>2)+1; offset = (uint32_t)(h>>8); hb = 5; }
        if (ip + hb > n) return 0;
        ip += hb;
        if (offset == 0 || offset > opos || opos + len > ulen) return 0;
        srcp = opos - offset; kind = 2;
      }
      ops[nops] = {opos, srcp, len, kind};
      opos += len; nops++;
    }
    uint64_t done = 0; uint32_t frontier = 0;
    while (frontier < nops) {
      uint32_t fdst = ops[frontier].dst;
      bool any = false;
      uint64_t newly = 0;
      for (uint32_t i = 0; i < nops; i++) {
        if ((done >> i) & 1) continue;
        Op& o = ops[i];
        bool ready = (o.kind == 1) || (o.src + o.len <= fdst) || (i == frontier);
        if (!ready) continue;
        any = true; newly |= 1ull << i;
        {
          const uint8_t* sbase = o.kind == 1 ? in : out;
          uint32_t offset = o.kind == 1 ? 0xffffffffu : o.dst - o.src;
          uint32_t t = 0;
          if (offset >= 16) {
            for (; t + 16 <= o.len; t += 16) {
              uint64_t a = ld64(sbase + o.src + t), b = ld64(sbase + o.src + t + 8);
              st64(out + o.dst + t, a); st64(out + o.dst + t + 8, b);
            }
            for (; t < o.len; t++) out[o.dst + t] = sbase[o.src + t];
          } else if (offset >= 8) {
            for (; t + 8 <= o.len; t += 8) st64(out + o.dst + t, ld64(out + o.src + t));
            for (; t < o.len; t++) out[o.dst + t] = out[o.src + t];
          } else {
            uint32_t p = o.dst, src = o.src, end = o.dst + o.len;
            while (p < end) {
              uint32_t d = p - src;
              if (end - p < 8) { for (; p < end; p++) out[p] = out[p - offset]; break; }
              if (d < 8) {
                st64(out + p, ld64(out + src));
                p += d < end - p ? d : end - p;
              } else {
                uint32_t dist = d;
                for (; p + 8 <= end; p += 8) st64(out + p, ld64(out + p - dist));
                for (; p < end; p++) out[p] = out[p - offset];
                break;
              }
            }
          }
        }
      }
      if (!any) { printf("STALL\n"); return 0; }
      done |= newly;
      while (frontier < nops && ((done >> frontier) & 1)) frontier++;
    }
  }
  return opos == ulen ? ulen : 0;
}
