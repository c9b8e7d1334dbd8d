// quic_set.hip -- the packet layer of a QUIC connection set
// (BSSL_AMD_QUIC_SET, include/bssl_amd/tls.h): one batch of packets across many
// slots, each one direction of one key generation of one packet-number space
// of one connection.  A slot's IV, header-protection key and number (the next
// packet number S[c] on seal, expected[c] on open) live on the device
// (QuicSetSlot); packets [run_start[j], run_start[j+1]) belong to slot
// c = run_slot[j].  The run-to-slot frame -- the claim, the search, the
// failure rules, the advance of the packet number (seal only, saturating at
// 2^62) -- is set_runs.h's, in its strict form; quic_prepare.h has the
// per-packet body.
//
//   quic_set_prepare_kernel   one lane per packet: set_lane(), then
//                             key_index[i], run_of[i] and quic_seal_packet with
//                             S[c] + k or quic_open_packet with the slot's
//                             expected, IV and header-protection key.  That key
//                             differs lane by lane: the AES masks read their
//                             round keys from the lane's odd-stride LDS slot
//                             (set_lanes.h) beside the bank-replicated T-table,
//                             ChaCha20's key words come from the slot into
//                             registers
//   quic_set_protect_kernel   after a seal: quic_protect_kernel with the lane's
//                             own key; a failed packet's slot zeroed
//   quic_set_expected_kernel  after an open: out_lengths, and the maximum of
//                             the authenticated packet numbers + 1 of every run
//                             onto its slot (a segmented maximum within the
//                             wave, one atomicMax per wave and run)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "internal.h"
#include "quic_prepare.h"
#include "lane_frame.h"
#include "set_lanes.h"
#include "set_runs.h"
#include "wave_bytes.h"

namespace bssl_amd {
namespace {

constexpr int kThreads = kSetThreads;

// MASK: kDtlsMaskNone for a seal (no mask in this step), the suite's for an open.
template <int MASK>
__global__ __launch_bounds__(kThreads) void quic_set_prepare_kernel(QuicSetPrepare p) {
  __shared__ SetLds<MASK> L;
  if constexpr (dtls_mask_is_aes(MASK)) lane_fill_tables(L, kAesTables.te0, kThreads);
  const QuicPrepare &r = p.pk;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  // (Only a seal consumes packet numbers.)
  const SetLane l = set_lane(p.runs, p.slots, r.n, i, MASK == kDtlsMaskNone);
  const QuicSetSlot &sl = p.slots[l.c];
  // Every thread of the workgroup reaches the LDS fill.
  const uint32_t *hp = set_mask_key<MASK>(sl.hp, L);
  if (i >= r.n) return;
  p.runs.run_of[i] = l.ok ? (uint32_t)l.j + 1 : 0;
  p.runs.key_index[i] = l.ok ? l.c : 0;
  if (l.ok) {
    const TlsIv iv = {sl.iv_lo, sl.iv_hi};
    if constexpr (MASK == kDtlsMaskNone)
      quic_seal_packet(r, i, l.number, iv);
    else
      quic_open_packet<MASK>(r, i, iv, sl.pn, hp, L);
    return;
  }
  // A packet without a slot: the bulk kernel gives it status 0 (valid 0); its
  // scratch inputs are defined, and nothing of it is written to `out` here (a
  // sealed one's slot is zeroed by the protect step).
  const QuicPacket k = quic_packet(r.offsets, r.lengths, r.packet_stride, r.packet_len,
                                   r.pn_offsets, r.pn_offset, i);
  const TlsIv zero = {0, 0};
  if (r.packet_numbers) r.packet_numbers[i] = 0;
  if (MASK != kDtlsMaskNone) {
    if (r.header_lengths) r.header_lengths[i] = 0;
    r.pns[i] = 0;
  }
  quic_describe(r, i, k, false, 0, 0, zero, 0);
}

template <int MASK>
__global__ __launch_bounds__(kThreads) void quic_set_protect_kernel(QuicProtect p,
                                                                    const QuicSetSlot *slots,
                                                                    uint32_t num_slots,
                                                                    const uint32_t *key_index) {
  __shared__ SetLds<MASK> L;
  if constexpr (dtls_mask_is_aes(MASK)) lane_fill_tables(L, kAesTables.te0, kThreads);
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < p.n;
  const bool ok = live && p.status[i] != 0;
  const uint32_t c = ok ? key_index[i] : 0;
  const uint32_t *hp = set_mask_key<MASK>(slots[c < num_slots ? c : 0].hp, L);
  uint64_t off = 0, len = 0;
  if (live) {
    off = p.offsets ? p.offsets[i] : i * p.packet_stride;
    len = p.lengths ? p.lengths[i] : p.packet_len;
    if (ok)
      quic_protect_packet<MASK>(p.out + off, len, p.body_offsets[i] - off, p.body_lengths[i],
                                p.tags + 16 * i, hp, L);
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

__global__ __launch_bounds__(kThreads) void quic_set_expected_kernel(QuicSetExpected p) {
  const QuicExpected &e = p.e;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool passed = i < e.n && e.status[i] != 0;
  if (i < e.n && e.out_lengths) e.out_lengths[i] = passed ? e.body_lengths[i] : 0;
  // (run + 1, packet number + 1) of a packet that counts.
  RunSeq v = {0, 0};
  if (passed) {
    v.r = p.run_of[i];  // 0: never contributes
    v.s = v.r ? e.pns[i] + 1 : 0;
  }
  // Runs are contiguous in index, so r does not decrease along the scan: the
  // last lane of each run's stretch holds the maximum of the run's packets in
  // this wave.
  v = wave_scan_max(v, lane);
  const uint32_t next_r = (uint32_t)__shfl_down((int)v.r, 1);
  if (v.r && v.r <= p.num_runs && (lane == 63 || next_r != v.r)) {
    const uint32_t won = p.run_won[v.r - 1];
    if (won && won <= p.num_slots)
      atomicMax(reinterpret_cast<unsigned long long *>(&p.slots[won - 1].pn),
                (unsigned long long)v.s);
  }
}

}  // namespace

int launch_quic_set_prepare(const QuicSetPrepare &p, int mask, void *stream) {
  if (p.pk.n == 0 || p.runs.num_runs == 0) return 0;
  if (p.pk.open && mask == kDtlsMaskNone) return 1;  // an open always has a mask
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((p.pk.n + kThreads - 1) / kThreads));
  return launch_set_prepare(p.runs, p.slots, p.pk.n, p.pk.open, s, [&] {
    // Only an open computes masks in this step.
    with_mask(p.pk.open ? mask : kDtlsMaskNone, [&](auto m) {
      hipLaunchKernelGGL(quic_set_prepare_kernel<decltype(m)::value>, grid, dim3(kThreads), 0, s, p);
    });
  });
}

int launch_quic_set_protect(const QuicProtect &m, const QuicSetSlot *slots, uint32_t num_slots,
                            const uint32_t *key_index, int mask, void *stream) {
  if (m.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((m.n + kThreads - 1) / kThreads));
  with_mask(mask, [&](auto k) {
    hipLaunchKernelGGL(quic_set_protect_kernel<decltype(k)::value>, grid, dim3(kThreads), 0, s, m,
                       slots, num_slots, key_index);
  });
  return (int)hipGetLastError();
}

int launch_quic_set_expected(const QuicSetExpected &p, void *stream) {
  if (p.e.n == 0 || p.num_runs == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(quic_set_expected_kernel, dim3((unsigned)((p.e.n + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, p);
  return (int)hipGetLastError();
}

}  // namespace bssl_amd
