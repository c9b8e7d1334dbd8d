// aes_tables.h -- the constant-time bank-replicated AES T-tables in LDS and the
// FIPS-197 cipher on them, shared by gcm_siv.hip and cbcmac.hip (DESIGN.md
// §4.8, §4.10, §4.12).  The workgroup's LDS structure (`LDS` below) holds
//   uint32_t t[256][2][32];   // T0 / T1, replica (lane & 31)
// filled from kAesTables at kernel start (entry e of the flat array:
// te0[e >> 6], rotated left by 8 when bit 5 of e is set).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bssl_amd {
namespace {

// AES tables: T0 and T1 = rotl8(T0), each replicated once per LDS bank (entry
// x of table t for lane l at t[x][t][l & 31], 64 KiB), so every lookup of a
// wave is bank-conflict free whatever the (secret) index -- the
// constant-time argument of gcm.hip's tables; T2/T3 are
// rot16(T0/T1), one rotate per column.  (Rounds 1/2 used four plain 1 KiB
// tables, whose bank conflicts depend on the data.)
struct Tables {
  uint32_t te0[256];
};

constexpr uint8_t cx_mul(uint8_t a, uint8_t b) {
  uint8_t p = 0;
  for (int i = 0; i < 8; i++) {
    if (b & 1) p ^= a;
    a = (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0));
    b >>= 1;
  }
  return p;
}

constexpr Tables make_tables() {
  Tables t{};
  for (int x = 0; x < 256; x++) {
    uint8_t inv = 1, base = (uint8_t)x;  // x^254
    for (int e = 254; e; e >>= 1) {
      if (e & 1) inv = cx_mul(inv, base);
      base = cx_mul(base, base);
    }
    if (!x) inv = 0;
    uint8_t s = inv, r = inv;
    for (int i = 0; i < 4; i++) {
      r = (uint8_t)((r << 1) | (r >> 7));
      s ^= r;
    }
    s ^= 0x63;
    // bytes (2s, s, s, 3s): the MixColumns column of a row-0 byte
    t.te0[x] = (uint32_t)cx_mul(s, 2) | ((uint32_t)s << 8) | ((uint32_t)s << 16) |
               ((uint32_t)cx_mul(s, 3) << 24);
  }
  return t;
}

__constant__ Tables kAesTables = make_tables();

__device__ __forceinline__ uint32_t rotl(uint32_t v, int n) {
  return __builtin_amdgcn_alignbit(v, v, 32 - n);
}

template <class LDS>
__device__ __forceinline__ uint32_t t0(const LDS &L, uint32_t x) {
  return L.t[x][0][threadIdx.x & 31];
}
template <class LDS>
__device__ __forceinline__ uint32_t t1(const LDS &L, uint32_t x) {
  return L.t[x][1][threadIdx.x & 31];
}
template <class LDS>
__device__ __forceinline__ uint32_t sbox(const LDS &L, uint32_t x) {
  return (t0(L, x) >> 8) & 0xff;
}

// FIPS-197 cipher on little-endian column words, from round R0 on (s = the
// state entering round R0); `rk` in LDS or global memory.
template <int NR, int R0, class LDS>
__device__ __forceinline__ uint4 aes_enc_from(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3,
                                              const uint4 *rk, const LDS &L) {
#pragma unroll
  for (int r = R0; r < NR; r++) {
    const uint4 k = rk[r];
    // T0[a] ^ T1[b] ^ T2[c] ^ T3[d] = T0[a] ^ T1[b] ^ rot16(T0[c] ^ T1[d])
    auto col = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t kk) {
      return t0(L, a & 0xff) ^ t1(L, (b >> 8) & 0xff) ^
             rotl(t0(L, (c >> 16) & 0xff) ^ t1(L, d >> 24), 16) ^ kk;
    };
    const uint32_t t0v = col(s0, s1, s2, s3, k.x), t1 = col(s1, s2, s3, s0, k.y),
                   t2 = col(s2, s3, s0, s1, k.z), t3 = col(s3, s0, s1, s2, k.w);
    s0 = t0v; s1 = t1; s2 = t2; s3 = t3;
  }
  const uint4 k = rk[NR];
  auto last = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return sbox(L, a & 0xff) | (sbox(L, (b >> 8) & 0xff) << 8) |
           (sbox(L, (c >> 16) & 0xff) << 16) | (sbox(L, d >> 24) << 24);
  };
  return make_uint4(last(s0, s1, s2, s3) ^ k.x, last(s1, s2, s3, s0) ^ k.y,
                    last(s2, s3, s0, s1) ^ k.z, last(s3, s0, s1, s2) ^ k.w);
}

template <int NR, class LDS>
__device__ __forceinline__ uint4 aes_enc(uint4 in, const uint4 *rk, const LDS &L) {
  return aes_enc_from<NR, 1>(in.x ^ rk[0].x, in.y ^ rk[0].y, in.z ^ rk[0].z, in.w ^ rk[0].w, rk,
                             L);
}

}  // namespace
}  // namespace bssl_amd
