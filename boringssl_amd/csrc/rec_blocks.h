// rec_blocks.h -- the blocks of the one-lane-per-record kernels (cbcmac.hip,
// ctr_hmac.hip, tls_cbc.hip): N blocks through the T-table AES of aes_tables.h
// together, and 16-byte blocks of records that start at any byte offset.  The
// frame those kernels share around their AEADs is lane_frame.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aes_tables.h"

namespace bssl_amd {
namespace {

__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) {
  return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
}

// N independent blocks through the cipher together, round by round (the
// rounds as a loop: the body already holds 16 N independent lookups).  rk: the
// schedule as 4 (NR + 1) words, in LDS (a lane's slot) or global memory
// (wave-uniform).
template <int NR, int N, class LDS>
__device__ __forceinline__ void aes_n(uint4 (&s)[N], const uint32_t *rk, const LDS &L) {
#pragma unroll
  for (int j = 0; j < N; j++) s[j] = xor4(s[j], make_uint4(rk[0], rk[1], rk[2], rk[3]));
#pragma unroll 1
  for (int r = 1; r < NR; r++) {
    const uint32_t k0 = rk[4 * r], k1 = rk[4 * r + 1], k2 = rk[4 * r + 2], k3 = rk[4 * r + 3];
#pragma unroll
    for (int j = 0; j < N; j++) {
      // T0[a] ^ T1[b] ^ T2[c] ^ T3[d] = T0[a] ^ T1[b] ^ rot16(T0[c] ^ T1[d])
      auto col = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t kk) {
        return t0(L, a & 0xff) ^ t1(L, (b >> 8) & 0xff) ^
               rotl(t0(L, (c >> 16) & 0xff) ^ t1(L, d >> 24), 16) ^ kk;
      };
      const uint4 v = s[j];
      s[j] = make_uint4(col(v.x, v.y, v.z, v.w, k0), col(v.y, v.z, v.w, v.x, k1),
                        col(v.z, v.w, v.x, v.y, k2), col(v.w, v.x, v.y, v.z, k3));
    }
  }
  const uint32_t k0 = rk[4 * NR], k1 = rk[4 * NR + 1], k2 = rk[4 * NR + 2], k3 = rk[4 * NR + 3];
#pragma unroll
  for (int j = 0; j < N; j++) {
    auto last = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
      return sbox(L, a & 0xff) | (sbox(L, (b >> 8) & 0xff) << 8) |
             (sbox(L, (c >> 16) & 0xff) << 16) | (sbox(L, d >> 24) << 24);
    };
    const uint4 v = s[j];
    s[j] = make_uint4(last(v.x, v.y, v.z, v.w) ^ k0, last(v.y, v.z, v.w, v.x) ^ k1,
                      last(v.z, v.w, v.x, v.y) ^ k2, last(v.w, v.x, v.y, v.z) ^ k3);
  }
}

// ---- record buffers: blocks as little-endian words of their bytes -----------

// min(16, the bytes of [0, total) from `at` on).
__device__ __forceinline__ uint32_t span16(uint64_t total, uint64_t at) {
  return at >= total ? 0u : total - at < 16 ? (uint32_t)(total - at) : 16u;
}

// The first n bytes of v (n <= 16), the rest zero.  (iov_dev.h has the same
// function: a file that includes it first, dtls.hip, takes that one.)
#ifndef BSSL_AMD_IOV_DEV_H
__device__ __forceinline__ uint4 mask_block(uint4 v, uint32_t n) {
  auto m = [&](uint32_t lo) {
    return n >= lo + 4 ? 0xffffffffu : n <= lo ? 0u : (1u << (8 * (n - lo))) - 1u;
  };
  return make_uint4(v.x & m(0), v.y & m(4), v.z & m(8), v.w & m(12));
}
#endif

// v with byte i (< 16) OR-ed with `val`.
__device__ __forceinline__ uint4 or_byte(uint4 v, uint32_t i, uint32_t val) {
  const uint32_t sh = val << (8 * (i & 3)), w = i >> 2;
  return make_uint4(v.x | (w == 0 ? sh : 0), v.y | (w == 1 ? sh : 0), v.z | (w == 2 ? sh : 0),
                    v.w | (w == 3 ? sh : 0));
}

// n (<= 16) bytes at p, zero-padded.  Records start at any byte offset: a
// full block that is not word-aligned is read as the five aligned words that
// hold it (each holds a byte of the block, so none is outside the buffer).
__device__ __forceinline__ uint4 load_block(const uint8_t *p, uint32_t n) {
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
  if (n == 16) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sh);
    const uint32_t a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
    if (sh == 0) return make_uint4(a0, a1, a2, a3);
    const uint32_t a4 = q[4];
    return make_uint4(__builtin_amdgcn_alignbyte(a1, a0, sh), __builtin_amdgcn_alignbyte(a2, a1, sh),
                      __builtin_amdgcn_alignbyte(a3, a2, sh), __builtin_amdgcn_alignbyte(a4, a3, sh));
  }
  uint4 v = make_uint4(0, 0, 0, 0);
  for (uint32_t i = 0; i < n; i++) v = or_byte(v, i, p[i]);
  return v;
}

// The first n (<= 16) bytes of v to p: whole words where p allows, bytes at
// the ends (never a byte outside [p, p + n)).
__device__ __forceinline__ void store_block(uint8_t *p, uint4 v, uint32_t n) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
  if (n == 16 && sh == 0) {
    uint32_t *q = reinterpret_cast<uint32_t *>(p);
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    return;
  }
  if (n == 16) {
    const uint32_t head = 4 - sh;  // bytes before the first aligned word
    uint32_t *q = reinterpret_cast<uint32_t *>(p + head);
    q[0] = __builtin_amdgcn_alignbyte(v.y, v.x, head);
    q[1] = __builtin_amdgcn_alignbyte(v.z, v.y, head);
    q[2] = __builtin_amdgcn_alignbyte(v.w, v.z, head);
    for (uint32_t i = 0; i < head; i++) p[i] = (uint8_t)(v.x >> (8 * i));
    for (uint32_t i = 16 - sh; i < 16; i++) p[i] = (uint8_t)(v.w >> (8 * (i & 3)));
    return;
  }
#pragma unroll
  for (uint32_t i = 0; i < 16; i++)
    if (i < n) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

template <typename T>
__device__ __forceinline__ T meta(const T *arr, uint64_t i, T dflt) {
  return arr ? arr[i] : dflt;
}

}  // namespace
}  // namespace bssl_amd
