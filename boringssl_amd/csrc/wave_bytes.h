// wave_bytes.h -- what a whole wave does to one record's bytes, shared by the
// kernels that frame the bulk AEAD kernels (tls_pad.hip, dtls.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bssl_amd {
namespace {

__device__ __forceinline__ uint64_t bcast64(uint64_t v, int lane) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

// The wave zeroes bytes [0, n) at p (wave-uniform): whole aligned 16-byte
// words where they lie inside, single bytes in the two words at the ends.
__device__ __forceinline__ void wave_zero(uint8_t *p, uint64_t n, int lane) {
  const uint64_t head = (uintptr_t)p & 15;
  uint8_t *base = p - head;
  for (uint64_t q = lane; 16 * q < head + n; q += 64) {
    const uint64_t lo = max(16 * q, head), hi = min(16 * q + 16, head + n);
    if (hi - lo == 16)
      *reinterpret_cast<uint4 *>(base + 16 * q) = make_uint4(0, 0, 0, 0);
    else
      for (uint64_t x = lo; x < hi; x++) base[x] = 0;
  }
}

}  // namespace
}  // namespace bssl_amd
