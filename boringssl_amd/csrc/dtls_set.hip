// dtls_set.hip -- the record layer of a DTLS association set
// (BSSL_AMD_DTLS_SET, include/bssl_amd/tls.h): one batch of records across many
// slots, each one direction of one epoch of one association.  A slot's fixed
// IV, epoch, record-number key, write sequence number and replay window live
// on the device (DtlsSetSlot); records [run_start[j], run_start[j+1]) belong
// to slot c = run_slot[j].  The run-to-slot frame -- the claim, the search,
// the failure rules, the advance of the write sequence number (seal only,
// saturating at 2^48) -- is set_runs.h's, in its strict form; dtls_prepare.h
// has the per-record body and the windows are dtls.hip's parallel form, one
// per slot.
//
//   dtls_set_prepare_kernel  one lane per record: set_lane(), then key_index[i],
//                            run_of[i] and dtls_prepare_record with the
//                            slot's epoch, IV, S[c] + k or window maximum and
//                            record-number key.  That key differs lane by lane:
//                            the AES masks read their round keys from the lane's
//                            odd-stride LDS slot (set_lanes.h) beside the
//                            bank-replicated T-table, ChaCha20's key words come
//                            from the slot into registers
//   dtls_set_mask_kernel     after a DTLS 1.3 seal: dtls_mask_kernel with the
//                            lane's own key
//   dtls_set_window_*        the replay windows, below
//
// The windows.  The sequential definition, per slot: for the run's records
// that authenticated, in index order, refuse record i if ShouldDiscard(s_i),
// else Record(s_i).  In parallel, with r_i = j + 1 the record's run and M0 its
// slot's maximum when the call runs, record i is accepted when it
// authenticated and
//   (a) no earlier authentic record of its run has its sequence number: a
//       table of record indices keyed by (r, s) -- atomicCAS from empty, and
//       atomicMin of the index where the resident record has the same key
//       (run_of and seqs do not change any more, so a slot's key never does);
//   (b) s_i > runmax_i or runmax_i - s_i < 256, with runmax_i = max(M0, s_k of
//       the authentic k < i of the same run).  run_start is non-decreasing (or
//       nothing authenticated), so r is non-decreasing over the authentic
//       records, and the plain exclusive prefix maximum of the pairs (r, s) in
//       lexicographic order -- (0, 0) for the others -- ends in the record's
//       own run exactly when that run has an earlier authentic record, whose
//       largest s it then carries; otherwise runmax_i = M0;
//   (c) s_i is not marked in the slot's window as the call found it.
// The slot's new maximum is the maximum over M0 and the run's authentic s
// (atomicMax per run, one per wave and run); the new map is the old one
// shifted by the growth, OR the accepted records within 255 of the new
// maximum.  For every run this is dtls.hip's form over that run's records
// alone, so a slot ends where the loop over one-association calls leaves it.
// Four launches: insert + workgroup maxima + run maxima; the scan of the
// workgroup maxima (one workgroup of 1024); the windows' shift (one thread per
// run); decide, mark, and zero what is newly refused.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "internal.h"
#include "dtls_prepare.h"
#include "lane_frame.h"
#include "set_lanes.h"
#include "set_runs.h"
#include "wave_bytes.h"

namespace bssl_amd {
namespace {

constexpr int kThreads = kSetThreads;

template <int MASK>
__global__ __launch_bounds__(kThreads) void dtls_set_prepare_kernel(DtlsSetPrepare p) {
  __shared__ SetLds<MASK> L;
  if constexpr (dtls_mask_is_aes(MASK)) lane_fill_tables(L, kAesTables.te0, kThreads);
  const DtlsPrepare &r = p.rec;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  // (Only a seal consumes sequence numbers.)
  const SetLane l = set_lane(p.runs, p.slots, r.n, i, !r.open);
  const DtlsSetSlot &sl = p.slots[l.c];
  // Every thread of the workgroup reaches the LDS fill.
  const uint32_t *sn = set_mask_key<MASK>(sl.sn, L);
  if (i >= r.n) return;
  p.runs.run_of[i] = l.ok ? (uint32_t)l.j + 1 : 0;
  p.runs.key_index[i] = l.ok ? l.c : 0;
  if (l.ok) {
    // (A DTLS 1.3 seal's flag is the pre-pass's, tls_pad.hip; an open's is
    // written by the body.)
    if (!r.open && !r.dtls13) r.valid[i] = 1;
    const TlsIv iv = {sl.iv_lo, sl.iv_hi};
    dtls_prepare_record<MASK>(r, i, sl.epoch, l.number, iv, sl.max_seq, sn, L);
    return;
  }
  // A record without a slot: the bulk kernel zeroes its outputs (valid 0); its
  // scratch inputs are defined, and a sealed record gets no header.
  r.valid[i] = 0;
  for (int b = 0; b < 12; b++) r.nonces[12 * i + b] = 0;
  for (uint32_t b = 0; b < r.ad_stride; b++) r.ad[(uint64_t)r.ad_stride * i + b] = 0;
  if (r.record_numbers) r.record_numbers[i] = 0;
  if (r.open) {
    r.seqs[i] = 0;
    if (r.ad_lengths) r.ad_lengths[i] = r.ad_stride;
    if (r.types_out) r.types_out[i] = 0;
  } else {
    if (r.out_lengths) r.out_lengths[i] = 0;
    for (uint32_t b = 0; b < r.prefix_len; b++) r.prefix[(uint64_t)r.prefix_len * i + b] = 0;
  }
}

template <int MASK>
__global__ __launch_bounds__(kThreads) void dtls_set_mask_kernel(DtlsMaskSeal p,
                                                                 const DtlsSetSlot *slots,
                                                                 uint32_t num_slots,
                                                                 const uint32_t *key_index) {
  __shared__ SetLds<MASK> L;
  if constexpr (dtls_mask_is_aes(MASK)) lane_fill_tables(L, kAesTables.te0, kThreads);
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool act = i < p.n && p.status[i] != 0;
  const uint32_t c = act ? key_index[i] : 0;
  const uint32_t *sn = set_mask_key<MASK>(slots[c < num_slots ? c : 0].sn, L);
  if (!act) return;
  const uint64_t len = p.lengths ? p.lengths[i] : p.record_len;
  const uint64_t off = p.offsets ? p.offsets[i] : i * p.record_stride;
  const uint32_t m = dtls_mask16<MASK>(dtls_sample(p.body + off, len, p.suffix + 16 * i), sn, L);
  uint8_t *pre = p.prefix + 5 * i;
  pre[1] ^= (uint8_t)m;
  pre[2] ^= (uint8_t)(m >> 8);
}

// ---- the windows ---------------------------------------------------------------

constexpr uint32_t kEmpty = ~0u;

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint64_t key_slot(RunSeq v, uint64_t slots) {
  const uint64_t x = v.s * 0x9e3779b97f4a7c15ull + (uint64_t)v.r * 0xc2b2ae3d27d4eb4full;
  return (x >> 20) & (slots - 1);
}

// The exclusive prefix maximum of v over a workgroup of THREADS threads ((0, 0)
// before the first); *total receives the maximum of all.  wr, ws: THREADS / 64
// words of LDS each.
template <int THREADS>
__device__ __forceinline__ RunSeq block_scan_max(RunSeq v, uint32_t *wr, uint64_t *ws,
                                                 RunSeq *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const RunSeq inc = wave_scan_max(v, lane);
  if (lane == 63) {
    wr[wave] = inc.r;
    ws[wave] = inc.s;
  }
  __syncthreads();
  RunSeq before = {0, 0}, all = {0, 0};
  for (int w = 0; w < THREADS / 64; w++) {
    const RunSeq x = {wr[w], ws[w]};
    if (w < wave) before = rs_max(before, x);
    all = rs_max(all, x);
  }
  const RunSeq up = rs_shfl_up(inc, 1);
  *total = all;
  return lane ? rs_max(before, up) : before;
}

// Record i's pair: its run and sequence number when it authenticated.
__device__ __forceinline__ RunSeq record_pair(const DtlsSetWindow &p, uint64_t i) {
  RunSeq v = {0, 0};
  if (i < p.w.n && p.w.status[i] != 0) {
    v.r = p.run_of[i];
    v.s = v.r ? p.w.seqs[i] : 0;
  }
  return v;
}

// Every authentic record enters its index under (run, sequence number); the
// runs' and the workgroup's maxima.
__global__ __launch_bounds__(256) void dtls_set_window_insert_kernel(DtlsSetWindow p) {
  __shared__ uint32_t wr[4];
  __shared__ uint64_t ws[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const RunSeq v = record_pair(p, i);
  if (v.r) {
    uint32_t *tab = reinterpret_cast<uint32_t *>(p.w.table);
    uint64_t h = key_slot(v, p.w.table_slots);
    for (uint64_t k = 0; k < p.w.table_slots; k++, h = (h + 1) & (p.w.table_slots - 1)) {
      const uint32_t e = atomicCAS(&tab[h], kEmpty, (uint32_t)i);
      if (e == kEmpty) break;
      if (e < p.w.n && p.run_of[e] == v.r && p.w.seqs[e] == v.s) {
        atomicMin(&tab[h], (uint32_t)i);
        break;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const RunSeq inc = wave_scan_max(v, lane);
  // r does not decrease along the scan: the last lane of each run's stretch
  // holds the maximum of the run's records in this wave.
  const uint32_t next_r = (uint32_t)__shfl_down((int)inc.r, 1);
  if (inc.r && inc.r <= p.num_runs && (lane == 63 || next_r != inc.r))
    atomicMax(reinterpret_cast<unsigned long long *>(&p.run_max[inc.r - 1]),
              (unsigned long long)inc.s);
  if (lane == 63) {
    wr[wave] = inc.r;
    ws[wave] = inc.s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    RunSeq all = {0, 0};
    for (int w = 0; w < 4; w++) all = rs_max(all, RunSeq{wr[w], ws[w]});
    p.block_r[blockIdx.x] = all.r;
    p.block_s[blockIdx.x] = all.s;
  }
}

// One workgroup: (block_r, block_s)[b] becomes the prefix maximum before
// workgroup b's first record.
__global__ __launch_bounds__(1024) void dtls_set_window_blocks_kernel(DtlsSetWindow p, uint64_t nb) {
  __shared__ uint32_t wr[16];
  __shared__ uint64_t ws[16];
  const uint64_t per = (nb + 1023) / 1024;
  const uint64_t lo = umin64(threadIdx.x * per, nb), hi = umin64(lo + per, nb);
  RunSeq mine = {0, 0};
  for (uint64_t b = lo; b < hi; b++) mine = rs_max(mine, RunSeq{p.block_r[b], p.block_s[b]});
  RunSeq all;
  RunSeq run = block_scan_max<1024>(mine, wr, ws, &all);
  for (uint64_t b = lo; b < hi; b++) {
    const RunSeq x = {p.block_r[b], p.block_s[b]};
    p.block_r[b] = run.r;
    p.block_s[b] = run.s;
    run = rs_max(run, x);
  }
}

// One thread per run: the slot of a run that won moves to its new maximum; its
// old state and the new maximum are kept in old[6 j ..] for the decisions.
__global__ void dtls_set_window_runs_kernel(DtlsSetWindow p) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.num_runs) return;
  const uint32_t won = p.run_won[j];
  if (won == 0) return;
  DtlsSetSlot &sl = p.slots[won - 1];
  const uint64_t m0 = sl.max_seq;
  const uint64_t m1 = umax64(m0, p.run_max[j]), shift = m1 - m0;
  uint64_t w[4], o[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; k++) w[k] = sl.bitmap[k];
  uint64_t *old = p.old + 6 * j;
  old[0] = m0;
  for (int k = 0; k < 4; k++) old[1 + k] = w[k];
  old[5] = m1;
  if (shift < 256) {  // Record(): map <<= shift (or reset)
    const int q = (int)(shift >> 6), r = (int)(shift & 63);
    for (int k = 3; k >= q; k--) {
      o[k] = w[k - q] << r;
      if (r && k - q - 1 >= 0) o[k] |= w[k - q - 1] >> (64 - r);
    }
  }
  sl.max_seq = m1;
  for (int k = 0; k < 4; k++) sl.bitmap[k] = o[k];
}

__global__ __launch_bounds__(256) void dtls_set_window_apply_kernel(DtlsSetWindow p) {
  __shared__ uint32_t wr[4];
  __shared__ uint64_t ws[4];
  const DtlsWindow &w = p.w;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const RunSeq v = record_pair(p, i);
  const bool passed = i < w.n && w.status[i] != 0;
  RunSeq all;
  const RunSeq before = rs_max(RunSeq{p.block_r[blockIdx.x], p.block_s[blockIdx.x]},
                               block_scan_max<256>(v, wr, ws, &all));
  // (A record that authenticated has a run that won: run_of is only set for
  // those; the checks keep every index in range all the same.)
  const uint32_t won = v.r && v.r <= p.num_runs ? p.run_won[v.r - 1] : 0;
  bool accept = false;
  if (won) {
    const uint64_t s = v.s;
    const uint64_t *old = p.old + 6 * (uint64_t)(v.r - 1);
    const uint64_t m0 = old[0], m1 = old[5];
    const uint64_t runmax = before.r == v.r ? umax64(m0, before.s) : m0;
    // (Every authentic record is in the table; the probe count is bounded all
    // the same, so that no state of the table can keep a lane here.)
    const uint32_t *tab = reinterpret_cast<const uint32_t *>(w.table);
    uint64_t h = key_slot(v, w.table_slots);
    bool first = false;
    for (uint64_t k = 0; k < w.table_slots; k++, h = (h + 1) & (w.table_slots - 1)) {
      const uint32_t e = tab[h];
      if (e == kEmpty || e >= w.n) break;
      if (p.run_of[e] == v.r && w.seqs[e] == s) {
        first = e == i;
        break;
      }
    }
    const bool inside = s > runmax || runmax - s < 256;  // ShouldDiscard's first half
    const uint64_t back = m0 - s;                        // (read when s <= m0)
    const bool seen = s <= m0 && back < 256 && ((old[1 + (back >> 6)] >> (back & 63)) & 1);
    accept = first && inside && !seen;
    if (accept && m1 - s < 256)
      atomicOr(reinterpret_cast<unsigned long long *>(&p.slots[won - 1].bitmap[(m1 - s) >> 6]),
               1ull << ((m1 - s) & 63));
  }
  uint64_t len = 0, off = 0;
  if (i < w.n) {
    len = w.lengths ? w.lengths[i] : w.record_len;
    off = w.offsets ? w.offsets[i] : i * w.record_stride;
  }
  const bool refuse = passed && !accept;
  if (i < w.n && w.set_lengths && w.out_lengths) w.out_lengths[i] = accept ? len : 0;
  if (refuse) {
    w.status[i] = 0;
    if (w.out_lengths) w.out_lengths[i] = 0;
    if (w.types) w.types[i] = 0;
  }
  // A refused record's output, record after record by the whole wave.
  unsigned long long todo = __ballot(refuse && len != 0);
  while (todo) {
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    wave_zero(w.out + bcast64(off, src), bcast64(len, src), lane);
  }
}

}  // namespace

int launch_dtls_set_prepare(const DtlsSetPrepare &p, int mask, void *stream) {
  if (p.rec.n == 0 || p.runs.num_runs == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((p.rec.n + kThreads - 1) / kThreads));
  return launch_set_prepare(p.runs, p.slots, p.rec.n, p.rec.open, s, [&] {
    // Only a DTLS 1.3 open computes masks in this step.
    with_mask(p.rec.open && p.rec.dtls13 ? mask : kDtlsMaskNone, [&](auto m) {
      hipLaunchKernelGGL(dtls_set_prepare_kernel<decltype(m)::value>, grid, dim3(kThreads), 0, s, p);
    });
  });
}

int launch_dtls_set_mask(const DtlsMaskSeal &m, const DtlsSetSlot *slots, uint32_t num_slots,
                         const uint32_t *key_index, int mask, void *stream) {
  if (m.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((m.n + kThreads - 1) / kThreads));
  with_mask(mask, [&](auto k) {
    hipLaunchKernelGGL(dtls_set_mask_kernel<decltype(k)::value>, grid, dim3(kThreads), 0, s, m,
                       slots, num_slots, key_index);
  });
  return (int)hipGetLastError();
}

int launch_dtls_set_window(const DtlsSetWindow &p, void *stream) {
  if (p.w.n == 0 || p.num_runs == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t nb = (p.w.n + 255) / 256;
  if (hipMemsetAsync(p.w.table, 0xff, 4 * p.w.table_slots, s) != hipSuccess) return 1;
  hipLaunchKernelGGL(dtls_set_window_insert_kernel, dim3((unsigned)nb), dim3(256), 0, s, p);
  hipLaunchKernelGGL(dtls_set_window_blocks_kernel, dim3(1), dim3(1024), 0, s, p, nb);
  hipLaunchKernelGGL(dtls_set_window_runs_kernel, dim3((unsigned)((p.num_runs + 255) / 256)),
                     dim3(256), 0, s, p);
  hipLaunchKernelGGL(dtls_set_window_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, p);
  return (int)hipGetLastError();
}

}  // namespace bssl_amd
