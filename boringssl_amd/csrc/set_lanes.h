// set_lanes.h -- what the kernels over sets of peers (dtls_set.hip,
// quic_set.hip) share beyond the run-to-slot frame (set_runs.h): the
// workgroup's LDS of a kernel that computes masks with a key per lane, and the
// prefix maximum of (run, number) pairs over a wave.
#ifndef BSSL_AMD_SET_LANES_H
#define BSSL_AMD_SET_LANES_H

#include <type_traits>

#include "internal.h"
#include "dtls_prepare.h"
#include "lane_frame.h"

namespace bssl_amd {
namespace {

constexpr int kSetThreads = 256;

// The workgroup's LDS of a kernel that computes masks with a key per lane: for
// the AES suites the T-table and 256 slots of 4 (NR + 1) + 1 words.
struct SetNoLds {
  uint32_t t[1][2][32];
};
template <int MASK>
constexpr int set_nr() {
  return MASK == kDtlsMaskAes256 ? 14 : 10;
}
template <int MASK>
using SetLds =
    std::conditional_t<dtls_mask_is_aes(MASK), LaneLds<set_nr<MASK>(), true, kSetThreads>, SetNoLds>;
static_assert(sizeof(SetLds<kDtlsMaskAes256>) == 64 * 1024 + kSetThreads * 61 * 4 &&
                  sizeof(SetLds<kDtlsMaskAes256>) <= 160 * 1024 &&
                  sizeof(SetLds<kDtlsMaskAes128>) <= 160 * 1024,
              "LDS per workgroup");

// The mask key of a lane from its slot's words (DtlsSetSlot::sn,
// QuicSetSlot::hp): the words themselves (ChaCha20: read into registers by the
// mask), or for AES the lane's LDS slot filled from them.  Every thread of the
// workgroup calls this (the barrier).
template <int MASK>
__device__ __forceinline__ const uint32_t *set_mask_key(const uint32_t *words, SetLds<MASK> &L) {
  if constexpr (dtls_mask_is_aes(MASK))
    return lane_round_keys<set_nr<MASK>(), true>(words, L);
  else
    return words;
}

// (run + 1, number), ordered lexicographically; (0, 0): none.
struct RunSeq {
  uint32_t r;
  uint64_t s;
};

__device__ __forceinline__ RunSeq rs_max(RunSeq a, RunSeq b) {
  return (b.r > a.r || (b.r == a.r && b.s > a.s)) ? b : a;
}

__device__ __forceinline__ RunSeq rs_shfl_up(RunSeq v, int d) {
  RunSeq u;
  u.r = (uint32_t)__shfl_up((int)v.r, d);
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v.s, d);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v.s >> 32), d);
  u.s = ((uint64_t)hi << 32) | lo;
  return u;
}

// The inclusive prefix maximum of v over the wave's lanes.
__device__ __forceinline__ RunSeq wave_scan_max(RunSeq v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const RunSeq u = rs_shfl_up(v, d);
    if (lane >= d) v = rs_max(v, u);
  }
  return v;
}

}  // namespace
}  // namespace bssl_amd

#endif
