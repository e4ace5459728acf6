// host entry points of the kernels' serial decoder (shared by dec_fuzz.cpp
// and corpus_check.cpp).  Include after dcw_snap_dec_lds.h.
#pragma once
static uint32_t snap_dec_lds_host(const uint8_t* in, uint32_t n, uint8_t* out,
                                  uint32_t cap) {
  return dcw::snap_dec_lds<1>(in, n, out, cap);
}
static uint32_t snap_dec_lds_host0(const uint8_t* in, uint32_t n, uint8_t* out,
                                   uint32_t cap) {
  return dcw::snap_dec_lds<0>(in, n, out, cap);
}
