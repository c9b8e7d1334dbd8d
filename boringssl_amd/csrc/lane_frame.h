// lane_frame.h -- the frame of the one-lane-per-record kernels (cbcmac.hip,
// ctr_hmac.hip, tls_cbc.hip): everything around "the record's
// bytes are in hand ... the tag is computed or compared", which is the AEAD
// itself and stays in its kernel.
//   device: the workgroup's LDS (LaneLds), its table fill, the record a lane
//           takes (lane_record), its round keys (lane_round_keys) and what a
//           finished record leaves behind (lane_finish);
//   host:   the launcher around the kernel launch (launch_lane_kernel) and the
//           nr x keyset fan-out (with_nr_keyset).
// What a kernel decides itself: its threads per workgroup (measured per
// kernel), the table it fills, its AEAD's conditions on a record, and whether
// small one-key batches take workgroups of half the size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "aes_tables.h"
#include "internal.h"
#include "rec_blocks.h"

namespace bssl_amd {
namespace {

// ---- device ------------------------------------------------------------------

// The workgroup's LDS: the 64 KiB bank-replicated table of aes_tables.h /
// aes_inv_tables.h and, for keysets, a slot per lane for its key's schedule.
// The slot stride in words is odd, so the 64 lanes' reads of word w fall in 64
// different banks.  THREADS: the kernel's largest workgroup, as large as
// 160 KiB allows for keysets.
template <int NR, bool KEYSET, int THREADS>
struct LaneLds {
  static constexpr int kStride = 4 * (NR + 1) + 1;  // odd: 45 or 61
  static constexpr int kSlotWords = KEYSET ? THREADS * kStride : 1;
  uint32_t t[256][2][32];  // T0 / T1 (or Td0 / Td1), replica (lane & 31)
  uint32_t slot[kSlotWords];
  static_assert(256 * 2 * 32 * 4 + kSlotWords * 4 <= (KEYSET ? 160 : 80) * 1024,
                "LDS per workgroup (one-key kernels: two workgroups per CU)");
  static_assert(kStride % 2 == 1,
                "odd slot stride: lane l's word w in bank (l * stride + w) % 64, all different");
};

// The table from its 256 words (kAesTables.te0 or kAesInvTables.td0); threads:
// those of the workgroup.  The caller's __syncthreads() is lane_round_keys'.
template <class LDS>
__device__ __forceinline__ void lane_fill_tables(LDS &L, const uint32_t *tab, uint32_t threads) {
  for (int e = threadIdx.x; e < 256 * 64; e += threads) {
    const uint32_t v = tab[e >> 6];
    (&L.t[0][0][0])[e] = ((e >> 5) & 1) ? rotl(v, 8) : v;
  }
}

// The record of a lane: position blockIdx.x * threads + threadIdx.x of the
// processing order.
struct LaneRecord {
  bool active;  // there is one
  uint64_t rec;
  uint64_t off, len, ad_off, ad_len;
  uint32_t kidx;
  // The common part of "this record is worked on": key_index in range and
  // valid[] set.  The kernel ANDs its AEAD's own conditions onto it, under
  // `if (active)`: the compiler then specialises the live path for what they
  // establish (cbcmac's loads for the nonce lengths), as it did for the
  // hand-written prologues.
  bool live;
};

template <bool KEYSET>
__device__ __forceinline__ LaneRecord lane_record(const BatchDesc &b, uint32_t threads) {
  LaneRecord r = {};
  const uint64_t pos = (uint64_t)blockIdx.x * threads + threadIdx.x;
  r.active = pos < b.num_records;
  r.rec = r.active ? (b.order ? (uint64_t)b.order[pos] : pos) : 0;
  r.live = r.active;
  if (r.active) {
    r.off = meta<uint64_t>(b.offsets, r.rec, r.rec * b.record_stride);
    r.len = meta<uint64_t>(b.lengths, r.rec, b.record_len);
    r.ad_off = meta<uint64_t>(b.ad_offsets, r.rec, r.rec * b.ad_stride);
    r.ad_len = meta<uint64_t>(b.ad_lengths, r.rec, b.ad_len);
    if (KEYSET) r.kidx = meta<uint32_t>(b.key_index, r.rec, 0u);
    r.live = r.kidx < b.num_keys && meta<uint8_t>(b.valid, r.rec, 1) != 0;
  }
  return r;
}

// Round keys: the key's own (rk: global, wave-uniform) or, for keysets, the
// lane's LDS slot, filled here.  Ends with the workgroup's barrier, which the
// table fill needs too.
template <int NR, bool KEYSET, class LDS>
__device__ __forceinline__ const uint32_t *lane_round_keys(const uint32_t *rk, LDS &L) {
  if constexpr (KEYSET) {
    uint32_t *slot = &L.slot[threadIdx.x * LDS::kStride];
    for (int w = 0; w < 4 * (NR + 1); w++) slot[w] = rk[w];
    rk = slot;
  }
  __syncthreads();
  return rk;
}

// The end of an active lane's record: its status, and a failed record's output
// and (seal) the first tag_bytes of its tag slot zero-filled
// (aead.cc.inc:132-139, 368-376, 539-547) -- a second pass over this record
// only.
template <bool OPEN>
__device__ __forceinline__ void lane_finish(const BatchDesc &b, uint64_t rec, int ok, uint64_t len,
                                            uint8_t *dst, uint32_t tag_bytes) {
  if (b.status) b.status[rec] = ok ? 1 : 0;
  if (ok) return;
  const uint4 z = make_uint4(0, 0, 0, 0);
  for (uint64_t o = 0; o < len; o += 16) store_block(dst + o, z, span16(len, o));
  if (!OPEN) {
    uint8_t *tagp = batch_tag(b, rec);
    for (uint32_t o = 0; o < tag_bytes; o += 16) store_block(tagp + o, z, span16(tag_bytes, o));
  }
}

// ---- host --------------------------------------------------------------------

// f(std::integral_constant<int, NR>, std::bool_constant<KEYSET>) for the
// batch's schedule length (nr: 10 or 14) and kind of key material.
template <class F>
void with_nr_keyset(int nr, bool keyset, F &&f) {
  using N10 = std::integral_constant<int, 10>;
  using N14 = std::integral_constant<int, 14>;
  if (nr == 14)
    keyset ? f(N14{}, std::true_type{}) : f(N14{}, std::false_type{});
  else
    keyset ? f(N10{}, std::true_type{}) : f(N10{}, std::false_type{});
}

// Everything around the launch of a one-lane-per-record kernel.  supported:
// the kernel exists for this nr (and hash).  threads: the workgroup of the
// instantiation that launch() picks.  half_rule: a one-key batch too small to
// give every CU a full workgroup takes workgroups of half the size, on twice
// as many CUs (ctr_hmac, 64K x 16 KiB: 171 workgroups instead of 86, 242 GB/s
// instead of 181).  launch(batch with its processing order, grid, threads,
// stream) launches the kernel.  Returns 0, 1 (not supported by these kernels),
// 2 (no memory for the order) or a HIP error code.
template <class Launch>
int launch_lane_kernel(const BatchDesc &b, bool supported, unsigned threads, bool half_rule,
                       void *stream, const KernelEvents *ev, Launch &&launch) {
  if (b.extra || b.extra_len || b.iovecs) return 1;
  if (!supported) return 1;
  if (b.num_records == 0) return 0;
  if (half_rule && !b.key_index && b.num_records < (uint64_t)threads * (uint64_t)device_cu_count())
    threads /= 2;
  const uint64_t grid = (b.num_records + threads - 1) / threads;
  if (grid > 0x7fffffffu) return 1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  BatchDesc bo = b;  // with the processing order of a ragged batch
  uint32_t *order = nullptr;
  if (wants_length_order(b)) {
    if (bssl_amd::scratch_alloc(reinterpret_cast<void **>(&order), (b.num_records + 128) * sizeof(uint32_t),
                       s) != hipSuccess)
      return 2;
    const int orc = build_length_order(b.lengths, b.num_records, order, order + b.num_records, s);
    if (orc) {
      bssl_amd::scratch_free(order, s);
      return orc;
    }
    bo.order = order;
  }
  if (ev) hipEventRecord(reinterpret_cast<hipEvent_t>(ev->start), s);
  launch(bo, (unsigned)grid, threads, s);
  const int rc = (int)hipGetLastError();
  if (ev) hipEventRecord(reinterpret_cast<hipEvent_t>(ev->stop), s);
  if (order) bssl_amd::scratch_free(order, s);
  return rc;
}

}  // namespace
}  // namespace bssl_amd
