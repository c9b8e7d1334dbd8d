// set_runs.h -- the run-to-slot frame of the kernels over sets of peers
// (tls_set.hip, dtls_set.hip, quic_set.hip).  A batch names its peers by runs
// (SetRuns, internal.h): records [run_start[j], run_start[j+1]) belong to slot
// c = run_slot[j] and get the numbers S[c], S[c] + 1, ... in record order,
// S[c] being the slot's counter on the device.  Three launches per call, in
// stream order (launch_set_prepare):
//
//   set_claim_kernel    one thread per run: a non-empty run of a slot in range
//                       writes ~j into the slot's claim word with atomicMax, so
//                       the lowest j wins -- deterministic, whatever the
//                       scheduling; a strict frame also checks run_start --
//                       non-decreasing, from 0 to n -- into the flag word
//   the prepare kernel  the layer's own, one lane per record: set_lane() finds
//                       the record's run (binary search over run_start),
//                       applies the failure rules and gives the record its
//                       number; the layer's body or its fill for a record
//                       without a slot follows
//   set_advance_kernel  one thread per run: the run that won a live slot
//                       advances the counter by its record count, saturating
//                       one past the layer's maximum number, and clears the
//                       claim word for the next call; a strict frame notes the
//                       winner in run_won[j]
//
// Nothing outside the batch's arrays is read or written, whatever run_start
// and run_slot hold: run_start's values are only compared with record indices
// (nothing is indexed by them), a record is worked on only when
// run_start[j] <= i < run_start[j+1] for the j the search returns (always below
// num_runs), and a slot is touched only when run_slot[j] < num_slots.  With the
// flag of a strict frame set no record is worked on at all.
//
// What differs between the layers is SetFrame<Slot>, all at compile time:
//   kNumber        the slot's counter field
//   kMaxNumber     the largest number a record may get; the counter rests one
//                  past it when the slot is exhausted
//   kStrict        a malformed run_start fails every record of the call (flag),
//                  and the batch keeps run_of / run_won for the steps after the
//                  bulk kernels.  The TLS set is laxer (bssl_amd/tls.h) and has
//                  none of the three arrays: they are never touched for it
//   kOpenAdvances  an open consumes numbers as a seal does (TLS: the implicit
//                  sequence number); otherwise only a seal advances the counter
#ifndef BSSL_AMD_SET_RUNS_H
#define BSSL_AMD_SET_RUNS_H

#include "internal.h"

namespace bssl_amd {
namespace {

template <class Slot>
struct SetFrame;
template <>
struct SetFrame<TlsSetConn> {
  static constexpr uint64_t TlsSetConn::*kNumber = &TlsSetConn::seq;
  // (tls_record.cc:302-306; e_aes.cc.inc:1087: 2^64 - 1 is never used.)
  static constexpr uint64_t kMaxNumber = UINT64_MAX - 1;
  static constexpr bool kStrict = false;
  static constexpr bool kOpenAdvances = true;
};
template <>
struct SetFrame<DtlsSetSlot> {
  static constexpr uint64_t DtlsSetSlot::*kNumber = &DtlsSetSlot::seq;
  static constexpr uint64_t kMaxNumber = kDtlsMaxSequence;  // HasNext, dtls_record.cc:500-505
  static constexpr bool kStrict = true;
  static constexpr bool kOpenAdvances = false;
};
template <>
struct SetFrame<QuicSetSlot> {
  static constexpr uint64_t QuicSetSlot::*kNumber = &QuicSetSlot::pn;
  static constexpr uint64_t kMaxNumber = kQuicMaxPacketNumber;
  static constexpr bool kStrict = true;
  static constexpr bool kOpenAdvances = false;
};

// The records of run j: run_start[j+1] - run_start[j], 0 for a decreasing pair.
__device__ __forceinline__ uint64_t run_count(const SetRuns &r, uint64_t j) {
  const uint64_t lo = r.run_start[j], hi = r.run_start[j + 1];
  return hi > lo ? hi - lo : 0;
}

// n: the records of the batch.
template <class Slot>
__global__ void set_claim_kernel(SetRuns r, Slot *slots, uint64_t n) {
  using F = SetFrame<Slot>;
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= r.num_runs) return;
  const uint64_t lo = r.run_start[j], hi = r.run_start[j + 1];
  if constexpr (F::kStrict)
    if (hi < lo || (j == 0 && lo != 0) || (j + 1 == r.num_runs && hi != n)) atomicOr(r.flag, 1u);
  const uint32_t c = r.run_slot[j];
  if (c >= r.num_slots || hi <= lo) return;  // an empty run claims nothing
  atomicMax(&slots[c].claim, ~(uint32_t)j);
}

// What set_lane() finds for record i.  ok: the record has a slot and a number.
// j, start: its run and the run's first record (when the run was found).  c:
// the slot the lane read -- its run's when that is in range, else 0 -- so
// slots[c] is always inside the set; a record with !ok is none of c's.
// number: S[c] + (i - start) when the caller asked for one and ok, else
// undefined or 0.
struct SetLane {
  bool ok;
  uint64_t j, start;
  uint32_t c;
  uint64_t number;
};

// The head of every prepare kernel, for record i of n (i may be past the
// batch: then !ok and nothing but slots[0] is read, so that a whole workgroup
// can go on to a barrier).  numbered: the record consumes a number of its slot
// -- the overflow rule applies, record by record.
template <class Slot>
__device__ __forceinline__ SetLane set_lane(const SetRuns &r, const Slot *slots, uint64_t n,
                                            uint64_t i, bool numbered) {
  using F = SetFrame<Slot>;
  SetLane l = {i < n, 0, 0, 0, 0};
  if constexpr (F::kStrict) l.ok = l.ok && *r.flag == 0;
  if (l.ok) {
    // The last run that starts at or before record i (run_start is
    // non-decreasing in a well-formed batch; empty runs share their start with
    // the next run and are passed over).
    uint64_t lo = 0, hi = r.num_runs;  // the answer is in [lo, hi)
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (r.run_start[mid] <= i)
        lo = mid;
      else
        hi = mid;
    }
    l.j = lo;
    l.start = r.run_start[lo];
    l.ok = l.start <= i && i < r.run_start[lo + 1];
  }
  if (l.ok) {
    const uint32_t c = r.run_slot[l.j];
    l.ok = c < r.num_slots;
    if (l.ok) l.c = c;
  }
  const Slot &sl = slots[l.c];
  // Live, and this run is the slot's first in the call.
  if (l.ok) l.ok = sl.live == 1 && sl.claim == ~(uint32_t)l.j;
  if (l.ok && numbered) {
    const uint64_t k = i - l.start, s0 = sl.*F::kNumber;
    l.ok = s0 <= F::kMaxNumber && k <= F::kMaxNumber - s0;
    l.number = s0 + k;
  }
  return l;
}

// open: the call's direction.
template <class Slot>
__global__ void set_advance_kernel(SetRuns r, Slot *slots, int open) {
  using F = SetFrame<Slot>;
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= r.num_runs) return;
  const uint32_t c = r.run_slot[j];
  const uint64_t cnt = run_count(r, j);
  uint32_t won = 0;
  if (c < r.num_slots && cnt != 0) {
    Slot &sl = slots[c];
    // Only the winner touches the slot, so no other thread of this launch
    // reads or writes what it writes.
    if (sl.claim == ~(uint32_t)j) {
      bool live = sl.live == 1;
      if constexpr (F::kStrict) live = live && *r.flag == 0;
      if (live) {
        won = c + 1;
        const uint64_t s0 = sl.*F::kNumber;
        if ((F::kOpenAdvances || !open) && s0 <= F::kMaxNumber)
          sl.*F::kNumber = cnt > F::kMaxNumber + 1 - s0 ? F::kMaxNumber + 1 : s0 + cnt;
      }
      sl.claim = 0;
    }
  }
  if constexpr (F::kStrict) r.run_won[j] = won;
}

// The three launches of a call over n records; `prepare` launches the layer's
// prepare kernel on s.  0 or a HIP error code.
template <class Slot, class Prepare>
int launch_set_prepare(const SetRuns &r, Slot *slots, uint64_t n, int open, hipStream_t s,
                       Prepare &&prepare) {
  const dim3 run_grid((unsigned)((r.num_runs + 255) / 256));
  hipLaunchKernelGGL(set_claim_kernel<Slot>, run_grid, dim3(256), 0, s, r, slots, n);
  prepare();
  hipLaunchKernelGGL(set_advance_kernel<Slot>, run_grid, dim3(256), 0, s, r, slots, open);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace bssl_amd

#endif
