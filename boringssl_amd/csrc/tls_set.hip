// tls_set.hip -- the record layer of a TLS connection set (BSSL_AMD_TLS_SET,
// include/bssl_amd/tls.h): one batch of records across many connections of
// one cipher suite.  The per-connection fixed IVs and sequence numbers live on
// the device (TlsSetConn); the run-to-slot frame -- the claim, the search, the
// failure rules, the advance -- is set_runs.h's, in its lax form with maximum
// number 2^64 - 2, so the counter saturates at 2^64 - 1.  What is here is the
// prepare kernel's tail: for a record with a sequence number what
// tls_prepare_kernel writes (tls_prepare.h), for the others the fill.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "set_runs.h"
#include "tls_prepare.h"

namespace bssl_amd {
namespace {

__global__ void tls_set_prepare_kernel(TlsSetPrepare p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.rec.n) return;
  // (An open consumes sequence numbers as a seal does.)
  const SetLane l = set_lane(p.runs, p.conns, p.rec.n, i, true);
  if (l.ok) {
    const TlsSetConn &cn = p.conns[l.c];
    const TlsIv iv = {cn.iv_lo, cn.iv_hi};
    p.runs.key_index[i] = l.c;
    // (A padded seal's flag is the pre-pass's, tls_pad.hip.)
    if (!(p.rec.padded && !p.rec.open)) p.rec.valid[i] = 1;
    tls_prepare_record(p.rec, i, l.number, iv);
    return;
  }
  // A record without a sequence number: the bulk kernel zeroes its outputs
  // (valid 0); its scratch inputs are defined, and a sealed record gets no
  // header.
  p.runs.key_index[i] = 0;
  p.rec.valid[i] = 0;
  for (int b = 0; b < 12; b++) p.rec.nonces[12 * i + b] = 0;
  for (uint32_t b = 0; b < p.rec.ad_stride; b++) p.rec.ad[(uint64_t)p.rec.ad_stride * i + b] = 0;
  if (!p.rec.open) {
    if (p.rec.padded && p.rec.out_lengths) p.rec.out_lengths[i] = 0;
    if (p.rec.tls13) p.rec.extra[i] = 0;
    for (uint32_t b = 0; b < p.rec.prefix_len; b++) p.rec.prefix[(uint64_t)p.rec.prefix_len * i + b] = 0;
  }
}

}  // namespace

int launch_tls_set_prepare(const TlsSetPrepare &p, void *stream) {
  if (p.rec.n == 0 || p.runs.num_runs == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return launch_set_prepare(p.runs, p.conns, p.rec.n, p.rec.open, s, [&] {
    hipLaunchKernelGGL(tls_set_prepare_kernel, dim3((unsigned)((p.rec.n + 255) / 256)), dim3(256),
                       0, s, p);
  });
}

}  // namespace bssl_amd
