// sha_compress.h -- the unrolled SHA-256 and SHA-1 compressions of the
// one-lane-per-record hash kernels (ctr_hmac.hip, tls_cbc.hip): the state in
// registers, the message schedule a rolling window of 16 words, the round
// constants literals.  Written from FIPS 180-4 (4.1.1, 4.1.2, 6.1.2, 6.2.2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha256_k.h"

namespace bssl_amd {
namespace {

__device__ __forceinline__ uint32_t rotr(uint32_t v, int n) {
  return __builtin_amdgcn_alignbit(v, v, n);
}
// Bits of x where m is set, of y elsewhere, and the XOR of three words: one
// v_bitop3_b32 each (gfx950's three-input boolean, which takes v_bfi_b32's
// place here).
__device__ __forceinline__ uint32_t bfi(uint32_t m, uint32_t x, uint32_t y) {
  return (m & x) | (~m & y);
}
__device__ __forceinline__ uint32_t xor3(uint32_t x, uint32_t y, uint32_t z) {
  return __builtin_amdgcn_bitop3_b32(x, y, z, 0x96);
}

// One compression: h += the 64 rounds over the block w (its sixteen big-endian
// words; used up as the schedule's rolling window).
__device__ __forceinline__ void sha256_compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 64; t++) {
    if (t >= 16) {
      const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
      w[t & 15] += xor3(rotr(w15, 7), rotr(w15, 18), w15 >> 3) + w[(t + 9) & 15] +
                   xor3(rotr(w2, 17), rotr(w2, 19), w2 >> 10);
    }
    const uint32_t t1 = hh + xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25)) + bfi(e, f, g) +
                        kSha256K[t] + w[t & 15];
    // Maj(a, b, c): c where a and b differ, else b.
    const uint32_t t2 = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22)) + bfi(a ^ b, c, b);
    hh = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
  h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// Four 16-byte blocks (little-endian words of their bytes) as the sixteen
// big-endian words of a SHA-256 block.
__device__ __forceinline__ void to_schedule(const uint4 (&v)[4], uint32_t (&w)[16]) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    w[4 * k] = __builtin_bswap32(v[k].x);
    w[4 * k + 1] = __builtin_bswap32(v[k].y);
    w[4 * k + 2] = __builtin_bswap32(v[k].z);
    w[4 * k + 3] = __builtin_bswap32(v[k].w);
  }
}

// SHA's padding (FIPS 180-4 5.1.1) of a message of `total` bytes, in its block
// w at byte offset `base`: 0x80 after the last byte where that falls into this
// block (the bytes past the message are zero already), and in the message's
// last block (`last`) its length `bits` at the end.
__device__ __forceinline__ void sha_padding(uint32_t (&w)[16], uint64_t total, uint64_t base,
                                            bool last, uint64_t bits) {
  if (total >= base && total - base < 64) {
    const uint32_t r = (uint32_t)(total - base);
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] |= (r >> 2) == (uint32_t)i ? 0x80000000u >> (8 * (r & 3)) : 0u;
  }
  if (last) {
    w[14] = (uint32_t)(bits >> 32);
    w[15] = (uint32_t)bits;
  }
}

// HMAC's outer block (RFC 2104): the inner digest (WORDS words: 5 for SHA-1,
// 8 for SHA-256) with SHA's padding; the opad block counts in the length.  The
// caller restarts its state from the key's outer state.
template <int WORDS>
__device__ __forceinline__ void hmac_outer_block(const uint32_t (&inner)[8], uint32_t (&w)[16]) {
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = i < WORDS ? inner[i] : 0;
  w[WORDS] = 0x80000000u;
  w[15] = 8 * (64 + 4 * WORDS);
}

// SHA-1 (FIPS 180-4 6.1.2): h[0..5) += the 80 rounds over the block w, used
// up as above.  (h has eight words so both hashes share their callers; SHA-1
// leaves the last three alone.)
__device__ __forceinline__ void sha1_compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
  for (int t = 0; t < 80; t++) {
    if (t >= 16)
      w[t & 15] = rotr(xor3(w[(t + 13) & 15], w[(t + 8) & 15], w[(t + 2) & 15]) ^ w[t & 15], 31);
    // Ch, Parity, Maj, Parity (Maj(b, c, d): d where b and c differ, else c).
    const uint32_t f = t < 20 ? bfi(b, c, d) : t < 40 ? xor3(b, c, d)
                       : t < 60 ? bfi(b ^ c, d, c) : xor3(b, c, d);
    const uint32_t k = t < 20 ? 0x5a827999u : t < 40 ? 0x6ed9eba1u
                       : t < 60 ? 0x8f1bbcdcu : 0xca62c1d6u;
    const uint32_t tmp = rotr(a, 27) + f + e + k + w[t & 15];
    e = d; d = c; c = rotr(b, 2); b = a; a = tmp;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}

}  // namespace
}  // namespace bssl_amd
