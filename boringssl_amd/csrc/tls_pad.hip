// tls_pad.hip -- TLS 1.3 record padding (RFC 8446 5.4) around the bulk AEAD
// kernels: the padded calls of include/bssl_amd/tls.h.
//
// A padded record's fragment is the encrypted TLSInnerPlaintext, content ||
// type || zeros, F bytes in one piece.  The AEAD work stays in the bulk
// kernels, which see plain records of F bytes; two kernels frame them:
//
//   tls13_pad_seal_kernel   before prepare and seal: per record the fragment
//                           length F and whether the record may be sealed
//                           (content <= 2^14, F <= 2^14 + 1, type != 0), the
//                           content copied to `out` when out != in, then the
//                           type byte and the zeros
//   tls13_pad_strip_kernel  after open: per authentic record the last non-zero
//                           byte of the fragment -- the type, and its index the
//                           content length (tls_record.cc:204-229)
//
// Both run one lane per record, and a lane finishes its record alone when the
// tail is short: at most 16 bytes of type and zeros to write, or a non-zero
// byte among the fragment's last 16.  The records left over are taken one
// after another by the whole wave, off the __ballot of unresolved lanes, in
// steps of 64 x 16 bytes: a record costs about F / 1024 wave steps, whatever
// padding a peer chose.  Memory is touched in aligned 16-byte words that hold
// at least one byte of the range at hand; the bytes outside it are masked on
// loads and never stored.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "wave_bytes.h"

namespace bssl_amd {
namespace {

constexpr uint64_t kTls13MaxFragment = kTlsMaxPlainLen + 1;  // content, type and padding

// A mask of bytes [a, b) of the 32-bit word that holds bytes [4w, 4w + 4) of a
// 16-byte word; a and b are positions in the 16-byte word, 0 <= a, b <= 16.
__device__ __forceinline__ uint32_t byte_mask(int w, int a, int b) {
  const int lo = min(max(a - 4 * w, 0), 4), hi = min(max(b - 4 * w, 0), 4);
  const uint32_t below_hi = hi >= 4 ? 0xffffffffu : (1u << (8 * hi)) - 1u;
  const uint32_t below_lo = lo >= 4 ? 0xffffffffu : (1u << (8 * lo)) - 1u;
  return hi > lo ? below_hi & ~below_lo : 0u;
}

// The position (0..15) of the last non-zero byte of bytes [a, b) of the
// 16-byte word v, or -1; *byte receives it.
__device__ __forceinline__ int last_nonzero(uint4 v, int a, int b, uint32_t *byte) {
  const uint32_t w[4] = {v.x & byte_mask(0, a, b), v.y & byte_mask(1, a, b),
                         v.z & byte_mask(2, a, b), v.w & byte_mask(3, a, b)};
  int pos = -1;
  uint32_t val = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int top = 3 - (__clz((int)w[k]) >> 3);  // (w[k] == 0: clz 32, top -1, unused)
    const bool hit = w[k] != 0;
    pos = hit ? 4 * k + top : pos;
    val = hit ? (w[k] >> (8 * (top & 3))) & 0xffu : val;
  }
  *byte = val;
  return pos;
}

// The wave copies n bytes (wave-uniform): in aligned 16-byte words when source
// and destination sit alike in theirs, else byte by byte across the lanes.
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, uint64_t n, int lane) {
  if ((((uintptr_t)dst ^ (uintptr_t)src) & 15) != 0) {
    for (uint64_t x = lane; x < n; x += 64) dst[x] = src[x];
    return;
  }
  const uint64_t head = (uintptr_t)dst & 15;
  uint8_t *db = dst - head;
  const uint8_t *sb = src - head;
  for (uint64_t q = lane; 16 * q < head + n; q += 64) {
    const uint64_t lo = max(16 * q, head), hi = min(16 * q + 16, head + n);
    if (hi - lo == 16)
      *reinterpret_cast<uint4 *>(db + 16 * q) = *reinterpret_cast<const uint4 *>(sb + 16 * q);
    else
      for (uint64_t x = lo; x < hi; x++) db[x] = sb[x];
  }
}

__global__ __launch_bounds__(256) void tls13_pad_seal_kernel(TlsPadSeal p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool active = i < p.n;
  uint64_t len = 0, frag = 0, off = 0;
  uint32_t type = 0;
  bool ok = false;
  if (active) {
    len = p.lengths ? p.lengths[i] : p.record_len;
    off = p.offsets ? p.offsets[i] : i * p.record_stride;
    type = p.types ? p.types[i] : p.type;
    // F = L + 1 + P in 64 bits: L <= 2^14 is checked first, P is below 2^32
    // and a block below 2^32 rounds L + 1 <= 2^14 + 1 up to less than 2^47.
    ok = len <= kTlsMaxPlainLen && type != 0;
    if (ok) {
      frag = len + 1;
      if (p.pad_lengths) {
        frag += p.pad_lengths[i];
      } else if (p.pad_block > 1) {
        const uint64_t rem = frag % p.pad_block;
        frag = min(rem ? frag + (p.pad_block - rem) : frag, kTls13MaxFragment);
      }
      ok = frag <= kTls13MaxFragment;  // RFC 8446 5.4; tls_record.cc:204-209
    }
    // A failed record goes through the bulk kernel as its content alone, which
    // that kernel zeroes (valid 0): nothing past out + off + L is written.
    p.frag_len[i] = ok ? frag : len;
    p.valid[i] = ok ? 1 : 0;
    if (p.out_lengths) p.out_lengths[i] = ok ? frag : 0;
  }
  uint8_t *dst = p.out + off;
  const uint64_t tail = ok ? frag - len : 0;  // the type and the zeros
  // The common case: the lane writes its record's tail alone.
  if (ok) dst[len] = (uint8_t)type;
  if (tail <= 16)
    for (uint64_t x = 1; x < tail; x++) dst[len + x] = 0;
  // The rest, record after record by the whole wave: the content of a record
  // that is not sealed in place, and a longer run of zeros.
  const bool copy = p.in != p.out;
  unsigned long long todo = __ballot(ok && ((copy && len != 0) || tail > 16));
  while (todo) {
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const uint64_t o = bcast64(off, src), l = bcast64(len, src), t = bcast64(tail, src);
    if (copy) wave_copy(p.out + o, p.in + o, l, lane);
    if (t > 16) wave_zero(p.out + o + l + 1, t - 1, lane);
  }
}

__global__ __launch_bounds__(256) void tls13_pad_strip_kernel(TlsPadStrip p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool active = i < p.n;
  uint64_t frag = 0, off = 0;
  bool scan = false;
  if (active) {
    frag = p.lengths ? p.lengths[i] : p.record_len;
    off = p.offsets ? p.offsets[i] : i * p.record_stride;
    // Only what the bulk kernel accepted (the header checks of the prepare
    // step are in its `valid` flags, so 1 <= F <= 2^14 + 1 here).
    scan = p.status[i] != 0 && frag != 0 && frag <= kTls13MaxFragment;
  }
  // Positions count from the aligned 16-byte word that holds the fragment's
  // first byte: the fragment is [head, end).
  const uint8_t *base = p.out + off;
  const uint32_t head = (uint32_t)((uintptr_t)base & 15);
  base -= head;
  const uint32_t end = head + (uint32_t)(scan ? frag : 0);
  int found = -1;  // position of the last non-zero byte
  uint32_t type = 0;
  // The lane's own look at the last 16 bytes, [lo, end): one or two words.
  const uint32_t lo = end - head > 16 ? end - 16 : head;
  if (scan) {
    const uint32_t q1 = (end - 1) >> 4;
    const uint4 v1 = *reinterpret_cast<const uint4 *>(base + 16 * q1);
    const int k1 = last_nonzero(v1, (int)max(lo, 16 * q1) - (int)(16 * q1), (int)(end - 16 * q1), &type);
    if (k1 >= 0) {
      found = (int)(16 * q1) + k1;
    } else if (16 * q1 > lo) {
      const uint4 v0 = *reinterpret_cast<const uint4 *>(base + 16 * (q1 - 1));
      const int k0 = last_nonzero(v0, (int)lo - (int)(16 * (q1 - 1)), 16, &type);
      if (k0 >= 0) found = (int)(16 * (q1 - 1)) + k0;
    }
  }
  // Unresolved with bytes left below `lo`: the wave takes the records one by
  // one, 1 KiB per step downwards from `lo`, and stops at the first step with
  // a non-zero byte.
  unsigned long long todo = __ballot(scan && found < 0 && lo > head);
  while (todo) {
    const int src = 63 - __clzll(todo);
    todo &= ~(1ull << src);
    const uint8_t *b = reinterpret_cast<const uint8_t *>(bcast64((uint64_t)(uintptr_t)base, src));
    const uint32_t h = (uint32_t)__shfl((int)head, src), e = (uint32_t)__shfl((int)lo, src);
    int pos = -1;
    uint32_t val = 0;
    for (int top = (int)((e - 1) >> 4); top >= 0 && pos < 0; top -= 64) {
      const int q = top - lane;
      int k = -1;
      uint32_t byte = 0;
      if (q >= 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(b + 16 * q);
        k = last_nonzero(v, (int)h - 16 * q, (int)e - 16 * q, &byte);
      }
      const unsigned long long hits = __ballot(k >= 0);
      if (hits) {  // the lowest lane holds the highest word
        const int first = __ffsll(hits) - 1;
        pos = 16 * (top - first) + __shfl(k, first);
        val = (uint32_t)__shfl((int)byte, first);
      }
    }
    if (lane == src) {
      found = pos;
      type = val;
    }
  }
  if (active) {
    // An authentic fragment of nothing but zeros has no type
    // (tls_record.cc:220-225); its output is all zero as it is.
    const bool ok = found >= 0;
    p.types[i] = ok ? (uint8_t)type : 0;
    p.out_lengths[i] = ok ? (uint64_t)((uint32_t)found - head) : 0;
    if (scan && !ok) p.status[i] = 0;
  }
}

}  // namespace

int launch_tls13_pad_seal(const TlsPadSeal &p, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tls13_pad_seal_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s,
                     p);
  return (int)hipGetLastError();
}

int launch_tls13_pad_strip(const TlsPadStrip &p, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tls13_pad_strip_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s,
                     p);
  return (int)hipGetLastError();
}

}  // namespace bssl_amd
