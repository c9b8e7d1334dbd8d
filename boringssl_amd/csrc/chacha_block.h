// chacha_block.h -- one ChaCha20 block (RFC 8439 2.3) in a lane's registers,
// for the record layers' per-record extras: the CBC suites' explicit IVs
// (tls_records.hip) and the DTLS 1.3 record-number mask (dtls_prepare.h).  The
// bulk cipher is chacha.hip's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bssl_amd {
namespace {

// Words 0..3 of the block of input state `in` (constants, key, counter and
// nonce in words 0..3, 4..11, 12, 13..15): its first 16 bytes, little-endian.
__device__ __forceinline__ void chacha20_block_head(const uint32_t (&in)[16], uint32_t (&out)[4]) {
  uint32_t x[16];
  for (int k = 0; k < 16; k++) x[k] = in[k];
  auto rotl = [](uint32_t v, int c) { return (v << c) | (v >> (32 - c)); };
  auto qr = [&](int a, int b, int c, int d) {
    x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16);
    x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12);
    x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8);
    x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7);
  };
  for (int r = 0; r < 10; r++) {
    qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
    qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
  }
  for (int k = 0; k < 4; k++) out[k] = x[k] + in[k];
}

}  // namespace
}  // namespace bssl_amd
