// tls_set.hip -- the record layer of a TLS connection set (BSSL_AMD_TLS_SET,
// include/bssl_amd/tls.h): one batch of records across many connections of
// one cipher suite.  The per-connection fixed IVs and sequence numbers live on
// the device (TlsSetConn); records [run_start[j], run_start[j+1]) belong to
// connection c = run_connection[j] and get the sequence numbers S[c],
// S[c] + 1, ... in record order.  Three kernels per call, in stream order:
//
//   tls_set_claim_kernel    one thread per run: a non-empty run of a connection
//                           in range writes ~j into the connection's claim
//                           word with atomicMax, so the lowest j wins --
//                           deterministic, whatever the scheduling
//   tls_set_prepare_kernel  one thread per record: finds its run (binary
//                           search over run_start), applies the failure rules
//                           into valid[i], writes key_index[i], and for a
//                           record with a sequence number what
//                           tls_prepare_kernel writes (tls_prepare.h)
//   tls_set_advance_kernel  one thread per run: the run that won advances
//                           S[c] by its record count, saturating at 2^64 - 1,
//                           and clears the claim word for the next call
//
// Nothing outside the batch's arrays is read or written, whatever run_start
// holds: a record is worked on only when run_start[j] <= i < run_start[j+1]
// for the j the search returns, and j is always below num_runs.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "tls_prepare.h"

namespace bssl_amd {
namespace {

// The records of run j: run_start[j+1] - run_start[j], 0 for a decreasing pair.
__device__ __forceinline__ uint64_t run_count(const TlsSetPrepare &p, uint64_t j) {
  const uint64_t lo = p.run_start[j], hi = p.run_start[j + 1];
  return hi > lo ? hi - lo : 0;
}

__global__ void tls_set_claim_kernel(TlsSetPrepare p) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.num_runs) return;
  const uint32_t c = p.run_connection[j];
  if (c >= p.num_connections || run_count(p, j) == 0) return;  // an empty run claims nothing
  atomicMax(&p.conns[c].claim, ~(uint32_t)j);
}

__global__ void tls_set_prepare_kernel(TlsSetPrepare p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.rec.n) return;
  // The last run that starts at or before record i (run_start is
  // non-decreasing in a well-formed batch; empty runs share their start with
  // the next run and are passed over).
  uint64_t lo = 0, hi = p.num_runs;  // the answer is in [lo, hi)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (p.run_start[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t j = lo;
  const uint64_t start = p.run_start[j];
  bool ok = start <= i && i < p.run_start[j + 1];
  uint32_t c = 0;
  uint64_t seq = 0;
  TlsIv iv = {0, 0};
  if (ok) {
    c = p.run_connection[j];
    ok = c < p.num_connections;
  }
  if (ok) {
    const TlsSetConn &cn = p.conns[c];
    // Live, this run is the connection's first in the call, and the sequence
    // number neither wraps nor is 2^64 - 1 (tls_record.cc:302-306;
    // e_aes.cc.inc:1087).
    const uint64_t k = i - start;
    ok = cn.live == 1 && cn.claim == ~(uint32_t)j && k < UINT64_MAX - cn.seq;
    if (ok) {
      seq = cn.seq + k;
      iv.lo = cn.iv_lo;
      iv.hi = cn.iv_hi;
    }
  }
  if (ok) {
    p.key_index[i] = c;
    // (A padded seal's flag is the pre-pass's, tls_pad.hip.)
    if (!(p.rec.padded && !p.rec.open)) p.rec.valid[i] = 1;
    tls_prepare_record(p.rec, i, seq, iv);
    return;
  }
  // A record without a sequence number: the bulk kernel zeroes its outputs
  // (valid 0); its scratch inputs are defined, and a sealed record gets no
  // header.
  p.key_index[i] = 0;
  p.rec.valid[i] = 0;
  for (int b = 0; b < 12; b++) p.rec.nonces[12 * i + b] = 0;
  for (uint32_t b = 0; b < p.rec.ad_stride; b++) p.rec.ad[(uint64_t)p.rec.ad_stride * i + b] = 0;
  if (!p.rec.open) {
    if (p.rec.padded && p.rec.out_lengths) p.rec.out_lengths[i] = 0;
    if (p.rec.tls13) p.rec.extra[i] = 0;
    for (uint32_t b = 0; b < p.rec.prefix_len; b++) p.rec.prefix[(uint64_t)p.rec.prefix_len * i + b] = 0;
  }
}

__global__ void tls_set_advance_kernel(TlsSetPrepare p) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.num_runs) return;
  const uint32_t c = p.run_connection[j];
  if (c >= p.num_connections) return;
  const uint64_t cnt = run_count(p, j);
  TlsSetConn &cn = p.conns[c];
  // Only the winner touches the connection, so no other thread of this launch
  // reads or writes what it writes.
  if (cnt == 0 || cn.claim != ~(uint32_t)j) return;
  if (cn.live == 1) cn.seq = cnt > UINT64_MAX - cn.seq ? UINT64_MAX : cn.seq + cnt;
  cn.claim = 0;
}

}  // namespace

int launch_tls_set_prepare(const TlsSetPrepare &p, void *stream) {
  if (p.rec.n == 0 || p.num_runs == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 run_grid((unsigned)((p.num_runs + 255) / 256));
  hipLaunchKernelGGL(tls_set_claim_kernel, run_grid, dim3(256), 0, s, p);
  hipLaunchKernelGGL(tls_set_prepare_kernel, dim3((unsigned)((p.rec.n + 255) / 256)), dim3(256), 0,
                     s, p);
  hipLaunchKernelGGL(tls_set_advance_kernel, run_grid, dim3(256), 0, s, p);
  return (int)hipGetLastError();
}

}  // namespace bssl_amd
