// quic.hip -- QUIC packet protection (RFC 9001 5) around the bulk AEAD
// kernels: the kernels of BSSL_AMD_QUIC_AEAD (include/bssl_amd/tls.h).
//
// The AEAD work stays in the bulk kernels, which see plain records whose AD
// happens to lie in `out` right before the body; what makes a packet a QUIC
// packet is here, one lane per packet (quic_prepare.h):
//
//   quic_prepare_kernel   step 1.  Seal: the header into `out` with the
//                         packet-number length bits and field.  Open: the
//                         mask of the sample, the unmasked header into `out`,
//                         the packet number decoded against `expected`, the
//                         tag into the scratch.  Both: nonce, body offset and
//                         length, header length, valid
//   quic_protect_kernel   after a seal: the tag to the packet's end, the mask
//                         of the fresh ciphertext onto the header; a failed
//                         packet's slot zeroed
//   quic_expected_kernel  step 3 of an open: out_lengths, and the maximum of
//                         the authenticated packet numbers + 1 into `expected`
//                         (wave reduction, one atomic per workgroup)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "internal.h"
#include "quic_prepare.h"
#include "lane_frame.h"
#include "wave_bytes.h"

namespace bssl_amd {
namespace {

struct QuicNoLds {
  uint32_t t[1][2][32];
};
template <int MASK>
using QuicLds = std::conditional_t<dtls_mask_is_aes(MASK), LaneLds<10, false, 256>, QuicNoLds>;

template <int MASK>
__global__ __launch_bounds__(256) void quic_prepare_kernel(QuicPrepare p) {
  __shared__ QuicLds<MASK> L;
  if constexpr (dtls_mask_is_aes(MASK)) {
    lane_fill_tables(L, kAesTables.te0, 256);
    __syncthreads();
  }
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const TlsIv iv = TlsIv::from_bytes(p.iv);
  if constexpr (MASK == kDtlsMaskNone)
    quic_seal_packet(p, i, p.next_pn + i, iv);
  else
    quic_open_packet<MASK>(p, i, iv, p.state->expected, p.state->hp, L);
}

template <int MASK>
__global__ __launch_bounds__(256) void quic_protect_kernel(QuicProtect p) {
  __shared__ QuicLds<MASK> L;
  if constexpr (dtls_mask_is_aes(MASK)) {
    lane_fill_tables(L, kAesTables.te0, 256);
    __syncthreads();
  }
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < p.n;
  uint64_t off = 0, len = 0;
  bool ok = false;
  if (live) {
    off = p.offsets ? p.offsets[i] : i * p.packet_stride;
    len = p.lengths ? p.lengths[i] : p.packet_len;
    ok = p.status[i] != 0;
    if (ok)
      quic_protect_packet<MASK>(p.out + off, len, p.body_offsets[i] - off, p.body_lengths[i],
                                p.tags + 16 * i, p.state->hp, L);
    if (p.out_lengths) p.out_lengths[i] = ok ? len + 16 : 0;
  }
  // A failed packet's slot, packet after packet by the whole wave.
  unsigned long long todo = __ballot(live && !ok);
  while (todo) {
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    wave_zero(p.out + bcast64(off, src), bcast64(len, src) + 16, lane);
  }
}

__device__ __forceinline__ uint64_t quic_shfl_xor64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void quic_expected_kernel(QuicExpected p) {
  __shared__ uint64_t ws[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool passed = i < p.n && p.status[i] != 0;
  if (i < p.n && p.out_lengths) p.out_lengths[i] = passed ? p.body_lengths[i] : 0;
  uint64_t v = passed ? p.pns[i] + 1 : 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t u = quic_shfl_xor64(v, d);
    v = u > v ? u : v;
  }
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) v = ws[w] > v ? ws[w] : v;
    if (v) atomicMax(reinterpret_cast<unsigned long long *>(&p.state->expected), (unsigned long long)v);
  }
}

}  // namespace

int launch_quic_prepare(const QuicPrepare &p, int mask, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((p.n + 255) / 256));
  // Only an open computes masks in this step.
  with_mask(p.open ? mask : kDtlsMaskNone, [&](auto m) {
    hipLaunchKernelGGL(quic_prepare_kernel<decltype(m)::value>, grid, dim3(256), 0, s, p);
  });
  return (int)hipGetLastError();
}

int launch_quic_protect(const QuicProtect &p, int mask, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((p.n + 255) / 256));
  with_mask(mask, [&](auto m) {
    hipLaunchKernelGGL(quic_protect_kernel<decltype(m)::value>, grid, dim3(256), 0, s, p);
  });
  return (int)hipGetLastError();
}

int launch_quic_expected(const QuicExpected &p, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(quic_expected_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
  return (int)hipGetLastError();
}

}  // namespace bssl_amd
