// aes_inv_tables.h -- the inverse cipher of FIPS-197 5.3.5 (the equivalent
// inverse cipher) on bank-replicated T-tables in LDS, for tls_cbc.hip's open.
// The workgroup's LDS structure holds, exactly as for aes_tables.h,
//   uint32_t t[256][2][32];   // Td0 / Td1, replica (lane & 31)
// filled from kAesInvTables (entry e of the flat array: td0[e >> 6], rotated
// left by 8 when bit 5 of e is set), so t0 / t1 of aes_tables.h read it and
// the table-access constant-time argument of DESIGN.md 4.10 carries over:
// every lane reads its own bank whatever the (secret) index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aes_tables.h"

namespace bssl_amd {
namespace {

struct InvTables {
  uint32_t td0[256];
};

constexpr InvTables make_inv_tables() {
  const Tables enc = make_tables();
  uint8_t si[256] = {};
  for (int x = 0; x < 256; x++) si[(enc.te0[x] >> 8) & 0xff] = (uint8_t)x;
  InvTables t{};
  // bytes (0e s, 09 s, 0d s, 0b s), s = Si[x]: the InvMixColumns column of a
  // row-0 byte.  0e ^ 09 ^ 0d ^ 0b = 01, so the XOR of the four bytes is s.
  for (int x = 0; x < 256; x++) {
    const uint8_t s = si[x];
    t.td0[x] = (uint32_t)cx_mul(s, 0x0e) | ((uint32_t)cx_mul(s, 0x09) << 8) |
               ((uint32_t)cx_mul(s, 0x0d) << 16) | ((uint32_t)cx_mul(s, 0x0b) << 24);
  }
  return t;
}

__constant__ InvTables kAesInvTables = make_inv_tables();

// Si[x] from Td0[x]: no third table.
template <class LDS>
__device__ __forceinline__ uint32_t inv_sbox(const LDS &L, uint32_t x) {
  uint32_t v = t0(L, x);
  v ^= v >> 16;
  return (v ^ (v >> 8)) & 0xff;
}

// N independent blocks through the inverse cipher together, round by round:
// aes_n of rec_blocks.h mirrored.  rk: the equivalent-inverse schedule (round
// NR's key first, InvMixColumns applied to the middle rounds; key_setup.cc) as
// 4 (NR + 1) words, in LDS (a lane's slot) or global memory (wave-uniform).
template <int NR, int N, class LDS>
__device__ __forceinline__ void aes_dec_n(uint4 (&s)[N], const uint32_t *rk, const LDS &L) {
#pragma unroll
  for (int j = 0; j < N; j++) {
    s[j].x ^= rk[0]; s[j].y ^= rk[1]; s[j].z ^= rk[2]; s[j].w ^= rk[3];
  }
#pragma unroll 1
  for (int r = 1; r < NR; r++) {
    const uint32_t k0 = rk[4 * r], k1 = rk[4 * r + 1], k2 = rk[4 * r + 2], k3 = rk[4 * r + 3];
#pragma unroll
    for (int j = 0; j < N; j++) {
      // InvShiftRows: row i of column c comes from column c - i.
      auto col = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t kk) {
        return t0(L, a & 0xff) ^ t1(L, (b >> 8) & 0xff) ^
               rotl(t0(L, (c >> 16) & 0xff) ^ t1(L, d >> 24), 16) ^ kk;
      };
      const uint4 v = s[j];
      s[j] = make_uint4(col(v.x, v.w, v.z, v.y, k0), col(v.y, v.x, v.w, v.z, k1),
                        col(v.z, v.y, v.x, v.w, k2), col(v.w, v.z, v.y, v.x, k3));
    }
  }
  const uint32_t k0 = rk[4 * NR], k1 = rk[4 * NR + 1], k2 = rk[4 * NR + 2], k3 = rk[4 * NR + 3];
#pragma unroll
  for (int j = 0; j < N; j++) {
    auto last = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
      return inv_sbox(L, a & 0xff) | (inv_sbox(L, (b >> 8) & 0xff) << 8) |
             (inv_sbox(L, (c >> 16) & 0xff) << 16) | (inv_sbox(L, d >> 24) << 24);
    };
    const uint4 v = s[j];
    s[j] = make_uint4(last(v.x, v.w, v.z, v.y) ^ k0, last(v.y, v.x, v.w, v.z) ^ k1,
                      last(v.z, v.y, v.x, v.w) ^ k2, last(v.w, v.z, v.y, v.x) ^ k3);
  }
}

}  // namespace
}  // namespace bssl_amd
