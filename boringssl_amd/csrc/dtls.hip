// dtls.hip -- DTLS 1.2 / 1.3 record protection around the bulk AEAD kernels:
// the kernels of BSSL_AMD_DTLS_AEAD (include/bssl_amd/tls.h).
//
// The AEAD work stays in the bulk kernels, which see plain records; what makes
// a record a DTLS record is here:
//
//   dtls_prepare_kernel  step 1, one lane per record (dtls_prepare.h).  Seal:
//                        header, explicit nonce, nonce and AD from the
//                        context's own sequence numbers.  Open: the received
//                        header's checks; for DTLS 1.3 the record-number mask
//                        (RFC 9147 4.2.3: one AES or ChaCha20 block of the
//                        first 16 ciphertext bytes), the unmasked sequence
//                        bytes and reconstruct_seqnum against the window's
//                        maximum; nonce, AD, AD length
//   dtls_mask_kernel     after a DTLS 1.3 seal: the mask of the fresh
//                        ciphertext onto header bytes 1..2
//   dtls_window_*        step 3 of an open: the anti-replay window
//                        (DTLSReplayBitmap, dtls_record.cc:29-57) over the
//                        records that authenticated, in index order
//
// The window's sequential definition -- for i = 0..n-1: refuse record i if
// ShouldDiscard(s_i), else Record(s_i) -- in parallel form.  Record i is
// accepted when it authenticated and
//   (a) no earlier authentic record of the batch has its sequence number: a
//       hash table keyed by sequence number, atomicMin of the index;
//   (b) s_i > runmax_i or runmax_i - s_i < 256, where runmax_i is the window's
//       maximum when record i's turn comes: max(M0, s_j of authentic j < i),
//       an exclusive prefix maximum (a refused record's s_j changes nothing:
//       it is at most runmax_j);
//   (c) s_i is not marked in the window the batch started with (a bit that
//       (b) lets through is still inside the window: bits only leave at the
//       far end as the maximum grows).
// The new maximum is the maximum over M0 and all authentic s_i; the new map is
// the old one shifted by the growth, OR the accepted records within 255 of the
// new maximum.  Three launches: insert + workgroup maxima; the scan of the
// workgroup maxima and the window's shift (one workgroup of 1024); decide,
// mark, and zero what is newly refused.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "internal.h"
#include "dtls_prepare.h"
#include "lane_frame.h"
#include "wave_bytes.h"

namespace bssl_amd {
namespace {

// The workgroup's LDS of a kernel that computes masks: the bank-replicated
// T-table for the AES suites, nothing to speak of otherwise.
struct DtlsNoLds {
  uint32_t t[1][2][32];
};
template <int MASK>
using DtlsLds = std::conditional_t<dtls_mask_is_aes(MASK), LaneLds<10, false, 256>, DtlsNoLds>;

template <int MASK>
__global__ __launch_bounds__(256) void dtls_prepare_kernel(DtlsPrepare p) {
  __shared__ DtlsLds<MASK> L;
  if constexpr (dtls_mask_is_aes(MASK)) {
    lane_fill_tables(L, kAesTables.te0, 256);
    __syncthreads();
  }
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  dtls_prepare_record<MASK>(p, i, p.epoch, p.seq + i, TlsIv::from_bytes(p.fixed_iv), p.state->max_seq,
                            p.state->sn, L);
}

template <int MASK>
__global__ __launch_bounds__(256) void dtls_mask_kernel(DtlsMaskSeal p) {
  __shared__ DtlsLds<MASK> L;
  if constexpr (dtls_mask_is_aes(MASK)) {
    lane_fill_tables(L, kAesTables.te0, 256);
    __syncthreads();
  }
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n || p.status[i] == 0) return;
  const uint64_t len = p.lengths ? p.lengths[i] : p.record_len;
  const uint64_t off = p.offsets ? p.offsets[i] : i * p.record_stride;
  const uint32_t m =
      dtls_mask16<MASK>(dtls_sample(p.body + off, len, p.suffix + 16 * i), p.state->sn, L);
  uint8_t *pre = p.prefix + 5 * i;
  pre[1] ^= (uint8_t)m;
  pre[2] ^= (uint8_t)(m >> 8);
}

// ---- the window ---------------------------------------------------------------

constexpr unsigned long long kEmpty = ~0ull;

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t seq_slot(uint64_t s, uint64_t slots) {
  return ((s * 0x9e3779b97f4a7c15ull) >> 20) & (slots - 1);
}

// The inclusive prefix maximum of v over the wave's lanes.
__device__ __forceinline__ uint64_t wave_scan_max(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t u = shfl_up64(v, d);
    if (lane >= d) v = umax64(v, u);
  }
  return v;
}

// The exclusive prefix maximum of v over a workgroup of THREADS threads (0
// before the first); *total receives the maximum of all.  ws: THREADS / 64
// words of LDS.
template <int THREADS>
__device__ __forceinline__ uint64_t block_scan_max(uint64_t v, uint64_t *ws, uint64_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t inc = wave_scan_max(v, lane);
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (int w = 0; w < THREADS / 64; w++) {
    const uint64_t x = ws[w];
    if (w < wave) before = umax64(before, x);
    all = umax64(all, x);
  }
  const uint64_t up = shfl_up64(inc, 1);
  *total = all;
  return umax64(before, lane ? up : 0);
}

// Every authentic record enters its sequence number with its index; the
// workgroup's maximum.
__global__ __launch_bounds__(256) void dtls_window_insert_kernel(DtlsWindow p) {
  __shared__ uint64_t ws[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool passed = i < p.n && p.status[i] != 0;
  const uint64_t s = passed ? p.seqs[i] : 0;
  if (passed) {
    unsigned long long *tab = reinterpret_cast<unsigned long long *>(p.table);
    for (uint64_t h = seq_slot(s, p.table_slots);; h = (h + 1) & (p.table_slots - 1)) {
      const unsigned long long k = atomicCAS(&tab[2 * h], kEmpty, (unsigned long long)s);
      if (k == kEmpty || k == s) {
        atomicMin(&tab[2 * h + 1], (unsigned long long)i);
        break;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t inc = wave_scan_max(s, lane);
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) p.block_max[blockIdx.x] = umax64(umax64(ws[0], ws[1]), umax64(ws[2], ws[3]));
}

// One workgroup: block_max[b] becomes the window's maximum when workgroup b's
// first record has its turn; the window moves to the new maximum, its old
// state is kept in p.old for the decisions.
__global__ __launch_bounds__(1024) void dtls_window_blocks_kernel(DtlsWindow p, uint64_t nb) {
  __shared__ uint64_t ws[16];
  const uint64_t m0 = p.state->max_seq;
  const uint64_t per = (nb + 1023) / 1024;
  const uint64_t lo = umin64(threadIdx.x * per, nb), hi = umin64(lo + per, nb);
  uint64_t mine = 0;
  for (uint64_t b = lo; b < hi; b++) mine = umax64(mine, p.block_max[b]);
  uint64_t all;
  uint64_t run = umax64(m0, block_scan_max<1024>(mine, ws, &all));
  for (uint64_t b = lo; b < hi; b++) {
    const uint64_t x = p.block_max[b];
    p.block_max[b] = run;
    run = umax64(run, x);
  }
  if (threadIdx.x == 0) {
    const uint64_t m1 = umax64(m0, all), shift = m1 - m0;
    uint64_t w[4], o[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; k++) w[k] = p.state->bitmap[k];
    p.old[0] = m0;
    for (int k = 0; k < 4; k++) p.old[1 + k] = w[k];
    if (shift < 256) {  // Record(): map <<= shift (or reset)
      const int q = (int)(shift >> 6), r = (int)(shift & 63);
      for (int k = 3; k >= q; k--) {
        o[k] = w[k - q] << r;
        if (r && k - q - 1 >= 0) o[k] |= w[k - q - 1] >> (64 - r);
      }
    }
    p.state->max_seq = m1;
    for (int k = 0; k < 4; k++) p.state->bitmap[k] = o[k];
  }
}

__global__ __launch_bounds__(256) void dtls_window_apply_kernel(DtlsWindow p) {
  __shared__ uint64_t ws[4];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool passed = i < p.n && p.status[i] != 0;
  const uint64_t s = passed ? p.seqs[i] : 0;
  uint64_t all;
  const uint64_t runmax = umax64(p.block_max[blockIdx.x], block_scan_max<256>(s, ws, &all));
  const uint64_t m0 = p.old[0], m1 = p.state->max_seq;
  bool accept = false;
  if (passed) {
    // (Every authentic record is in the table; the probe count is bounded all
    // the same, so that no state of the table can keep a lane here.)
    uint64_t h = seq_slot(s, p.table_slots);
    for (uint64_t k = 1; p.table[2 * h] != s && k < p.table_slots; k++)
      h = (h + 1) & (p.table_slots - 1);
    const bool first = p.table[2 * h] == s && p.table[2 * h + 1] == i;
    const bool inside = s > runmax || runmax - s < 256;  // ShouldDiscard's first half
    const uint64_t back = m0 - s;                        // (read when s <= m0)
    const bool seen = s <= m0 && back < 256 && ((p.old[1 + (back >> 6)] >> (back & 63)) & 1);
    accept = first && inside && !seen;
    if (accept && m1 - s < 256)
      atomicOr(reinterpret_cast<unsigned long long *>(&p.state->bitmap[(m1 - s) >> 6]),
               1ull << ((m1 - s) & 63));
  }
  uint64_t len = 0, off = 0;
  if (i < p.n) {
    len = p.lengths ? p.lengths[i] : p.record_len;
    off = p.offsets ? p.offsets[i] : i * p.record_stride;
  }
  const bool refuse = passed && !accept;
  if (i < p.n && p.set_lengths && p.out_lengths) p.out_lengths[i] = accept ? len : 0;
  if (refuse) {
    p.status[i] = 0;
    if (p.out_lengths) p.out_lengths[i] = 0;
    if (p.types) p.types[i] = 0;
  }
  // A refused record's output, record after record by the whole wave.
  unsigned long long todo = __ballot(refuse && len != 0);
  while (todo) {
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    wave_zero(p.out + bcast64(off, src), bcast64(len, src), lane);
  }
}

}  // namespace

int launch_dtls_prepare(const DtlsPrepare &p, int mask, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((p.n + 255) / 256));
  // Only a DTLS 1.3 open computes masks in this step.
  with_mask(p.open && p.dtls13 ? mask : kDtlsMaskNone, [&](auto m) {
    hipLaunchKernelGGL(dtls_prepare_kernel<decltype(m)::value>, grid, dim3(256), 0, s, p);
  });
  return (int)hipGetLastError();
}

int launch_dtls_mask(const DtlsMaskSeal &p, int mask, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((p.n + 255) / 256));
  with_mask(mask, [&](auto m) {
    hipLaunchKernelGGL(dtls_mask_kernel<decltype(m)::value>, grid, dim3(256), 0, s, p);
  });
  return (int)hipGetLastError();
}

int launch_dtls_window(const DtlsWindow &p, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t nb = (p.n + 255) / 256;
  if (hipMemsetAsync(p.table, 0xff, 16 * p.table_slots, s) != hipSuccess) return 1;
  hipLaunchKernelGGL(dtls_window_insert_kernel, dim3((unsigned)nb), dim3(256), 0, s, p);
  hipLaunchKernelGGL(dtls_window_blocks_kernel, dim3(1), dim3(1024), 0, s, p, nb);
  hipLaunchKernelGGL(dtls_window_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, p);
  return (int)hipGetLastError();
}

}  // namespace bssl_amd
