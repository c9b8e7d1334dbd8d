// ctr_hmac.hip -- AES-128/256-CTR-HMAC-SHA256 seal / open over device-resident
// record batches: the reference's one encrypt-then-MAC AEAD, whose tag is a
// hash.
//
// Replaces aead_aes_ctr_hmac_sha256_sealv / _openv_detached
// (crypto/cipher/e_aesctrhmac.cc:180-254, with hmac_calculate and
// aead_aes_ctr_hmac_sha256_crypt, :124-178).  Written from FIPS 180-4
// (SHA-256), RFC 2104 (HMAC) and the construction that file states:
//   ciphertext = AES-CTR, counter block nonce || be32(0), be32(1), ...
//   tag = HMAC-SHA256(le64(ad_len) || le64(len) || nonce || ad ||
//                     zeros to a multiple of 64 || ciphertext)[0 .. tag_len)
// Design:
// * A record's SHA-256 chain cannot be split, so records are the unit of
//   parallelism: one lane per record, as in cbcmac.hip.
// * One loop per record over the 64-byte blocks its hash takes, with a single
//   compression in its body: the header block(s), then the ciphertext in one
//   pass -- four counter blocks through the T-table AES together
//   (aes_n<NR, 4>), XOR, store, hash -- with SHA's padding, then the outer
//   compression over the inner digest.  The keystream runs one step ahead of
//   the hash: a step's body computes the next step's keystream before it
//   compresses its own ciphertext, and the two are independent on seal and
//   open alike.  The AES is LDS lookups, the compression VALU work.
// * The compression (sha_compress.h) keeps the state in 8 registers and the
//   message schedule in a rolling window of 16, fully unrolled, the 64
//   constants literals.
// * One key: the round keys and both HMAC states are wave-uniform (scalar
//   loads).  Keysets: round keys in per-lane LDS slots with an odd stride in
//   words (cbcmac.hip); the two states are read from global memory once each.
// * Ragged batches are processed in the order of build_length_order.
#include <hip/hip_runtime.h>

#include "aes_tables.h"
#include "internal.h"
#include "rec_blocks.h"
#include "sha_compress.h"

namespace bssl_amd {
namespace {

// Threads per workgroup and the LDS slot stride (words) of a lane's round keys.
// One key: the kernels take 144 VGPRs, three waves per SIMD, and a CU takes
// them as one workgroup of twelve waves (the dispatcher placed no second
// workgroup of six waves beside the first: 1.5 waves per SIMD measured).
// kThreads is the largest workgroup; see launch_one.
// Keysets: as large as 160 KiB of LDS allows.
template <int NR, bool KEYSET>
struct Shape {
  static constexpr int kStride = 4 * (NR + 1) + 1;  // odd: 45 or 61
  static constexpr int kThreads = !KEYSET ? 768 : NR == 14 ? 384 : 512;
  static constexpr int kSlotWords = KEYSET ? kThreads * kStride : 1;
};

template <int NR, bool KEYSET>
struct Lds {
  uint32_t t[256][2][32];  // T0 / T1, replica (lane & 31)
  uint32_t slot[Shape<NR, KEYSET>::kSlotWords];
};
static_assert(sizeof(Lds<10, true>) <= 160 * 1024 && sizeof(Lds<14, true>) <= 160 * 1024 &&
                  sizeof(Lds<10, false>) <= 80 * 1024 && sizeof(Lds<14, false>) <= 80 * 1024,
              "LDS per workgroup");
static_assert(Shape<10, true>::kStride % 2 == 1 && Shape<14, true>::kStride % 2 == 1,
              "odd slot stride: lane l's word w in bank (l * stride + w) % 64, all different");

// min(16, the bytes of [0, total) from `at` on).
__device__ __forceinline__ uint32_t span16(uint64_t total, uint64_t at) {
  return at >= total ? 0u : total - at < 16 ? (uint32_t)(total - at) : 16u;
}

// One record per lane.
template <bool OPEN, int NR, bool KEYSET>
__global__ __launch_bounds__((Shape<NR, KEYSET>::kThreads)) void ctr_hmac_kernel(
    const CtrHmacKeyDev *__restrict__ keys, BatchDesc b) {
  using S = Shape<NR, KEYSET>;
  __shared__ Lds<NR, KEYSET> L;
  // (blockDim.x, not kThreads: launch_one gives small one-key batches smaller
  // workgroups.)
  for (int e = threadIdx.x; e < 256 * 64; e += blockDim.x) {
    const uint32_t v = kAesTables.te0[e >> 6];
    (&L.t[0][0][0])[e] = ((e >> 5) & 1) ? rotl(v, 8) : v;
  }
  const uint64_t pos = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = pos < b.num_records;
  const uint64_t rec = active ? (b.order ? (uint64_t)b.order[pos] : pos) : 0;
  uint64_t off = 0, len = 0, ad_off = 0, ad_len = 0;
  uint32_t kidx = 0;
  bool live = active;
  if (active) {
    off = meta<uint64_t>(b.offsets, rec, rec * b.record_stride);
    len = meta<uint64_t>(b.lengths, rec, b.record_len);
    ad_off = meta<uint64_t>(b.ad_offsets, rec, rec * b.ad_stride);
    ad_len = meta<uint64_t>(b.ad_lengths, rec, b.ad_len);
    if (KEYSET) kidx = meta<uint32_t>(b.key_index, rec, 0u);
    // e_aesctrhmac.cc:97, 190, 201, 226, 237.  A record of 2^36 bytes or more
    // (the 32-bit block counter would wrap) fails alone, status 0, as gcm.hip
    // treats its own limit; no test can allocate one.
    live = kidx < b.num_keys && meta<uint8_t>(b.valid, rec, 1) != 0 && b.nonce_len == 12 &&
           b.tag_len <= 32 && len <= kCtrHmacMaxInput;
  }
  // Round keys: the key's own (global, wave-uniform) or the lane's LDS slot.
  const CtrHmacKeyDev &K = keys[live ? kidx : 0];
  const uint32_t *rk = &K.rk[0][0];
  if constexpr (KEYSET) {
    uint32_t *slot = &L.slot[threadIdx.x * S::kStride];
    for (int w = 0; w < 4 * (NR + 1); w++) slot[w] = rk[w];
    rk = slot;
  }
  __syncthreads();

  const uint32_t M = b.tag_len;
  const uint8_t *src = b.in + off;
  uint8_t *dst = b.out + off;
  int ok = live;
  if (live) {
    const uint8_t *ad = b.ad + ad_off;
    const uint4 nw = load_block(b.nonces + rec * 12, 12);
    // The hash takes nH header blocks (28 bytes of lengths and nonce, the AD,
    // zeros to the block boundary), nM blocks of ciphertext with SHA's padding
    // (0x80 and the 64-bit length: one block more when len % 64 is 56..63),
    // and the outer block.
    const uint64_t nH = (ad_len + 28 + 63) / 64;
    // (len < 2^36: the message block numbers fit 32 bits.)
    const uint32_t nM = (uint32_t)(len / 64) + 1 + ((len & 63) >= 56 ? 1 : 0);
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = K.inner[i];
    // Counter blocks 4 q .. 4 q + 3: nonce || be32(counter).
    auto counters = [&](uint4(&s)[4], uint32_t q) {
#pragma unroll
      for (int k = 0; k < 4; k++)
        s[k] = make_uint4(nw.x, nw.y, nw.z, __builtin_bswap32(4 * q + k));
    };
    uint4 ks[4];
    counters(ks, 0);
    if (len) aes_n<NR, 4>(ks, rk, L);
    for (uint64_t t = 0; t < nH + nM + 1; t++) {
      uint32_t w[16];
      if (t < nH) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint64_t o = 64 * t + 16 * k;  // offset in the header
          if (o == 0) {
            v[k] = make_uint4((uint32_t)ad_len, (uint32_t)(ad_len >> 32), (uint32_t)len,
                              (uint32_t)(len >> 32));
          } else if (o == 16) {
            v[k] = make_uint4(nw.x, nw.y, nw.z, load_block(ad, ad_len < 4 ? (uint32_t)ad_len : 4u).x);
          } else {
            const uint32_t n = span16(ad_len, o - 28);
            v[k] = n ? load_block(ad + (o - 28), n) : make_uint4(0, 0, 0, 0);
          }
        }
        to_schedule(v, w);
      } else if (t < nH + nM) {
        // Message block q: a lane reads its 64 bytes before it writes them
        // (in-place batches), and open hashes what it read.
        const uint32_t q = (uint32_t)(t - nH);
        const uint64_t base = 64 * (uint64_t)q;
        uint4 v[4];
        uint32_t n[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          n[k] = span16(len, base + 16 * k);
          v[k] = n[k] ? load_block(src + base + 16 * k, n[k]) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint4 y = mask_block(xor4(v[k], ks[k]), n[k]);
          if (n[k]) store_block(dst + base + 16 * k, y, n[k]);
          if (!OPEN) v[k] = y;
        }
        to_schedule(v, w);
        // The next step's keystream, ahead of this step's compression.
        if (base + 64 < len) {
          counters(ks, q + 1);
          aes_n<NR, 4>(ks, rk, L);
        }
        // SHA's padding: 0x80 after the last byte, the length in bits at the
        // end of the last block.
        if (len >= base && len - base < 64) {
          const uint32_t r = (uint32_t)(len - base);
#pragma unroll
          for (int i = 0; i < 16; i++) w[i] |= (r >> 2) == (uint32_t)i ? 0x80000000u >> (8 * (r & 3)) : 0u;
        }
        if (q + 1 == nM) {
          const uint64_t bits = 8 * (64 + 64 * nH + len);  // the ipad block counts
          w[14] = (uint32_t)(bits >> 32);
          w[15] = (uint32_t)bits;
        }
      } else {
        // The outer hash: one block, the inner digest with its padding, from
        // the state after the opad block.
#pragma unroll
        for (int i = 0; i < 8; i++) {
          w[i] = h[i];
          h[i] = K.outer[i];
          w[8 + i] = 0;
        }
        w[8] = 0x80000000u;
        w[15] = 8 * (64 + 32);
      }
      sha256_compress(h, w);
    }
    // The tag: the first M bytes of the digest, as two blocks.
    uint8_t *tagp = batch_tag(b, rec);
    const uint32_t m0 = M < 16 ? M : 16u, m1 = M - m0;
    const uint4 lo = mask_block(make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]),
                                           __builtin_bswap32(h[2]), __builtin_bswap32(h[3])), m0);
    const uint4 hi = mask_block(make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]),
                                           __builtin_bswap32(h[6]), __builtin_bswap32(h[7])), m1);
    if constexpr (OPEN) {
      // All M bytes compared, no early exit (CRYPTO_memcmp): the XOR
      // differences OR-ed together.
      const uint4 t0v = xor4(mask_block(load_block(tagp, m0), m0), lo);
      uint4 t1v = make_uint4(0, 0, 0, 0);
      if (m1) t1v = xor4(mask_block(load_block(tagp + 16, m1), m1), hi);
      ok = (t0v.x | t0v.y | t0v.z | t0v.w | t1v.x | t1v.y | t1v.z | t1v.w) == 0;
    } else {
      store_block(tagp, lo, m0);
      if (m1) store_block(tagp + 16, hi, m1);
    }
  }
  if (!active) return;
  if (b.status) b.status[rec] = ok ? 1 : 0;
  if (!ok) {
    // A failed record's output (and the tag of a failed seal) zero-filled
    // (aead.cc.inc:132-139, 539-547): a second pass over this record only.
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint64_t o = 0; o < len; o += 16) store_block(dst + o, z, len - o < 16 ? (uint32_t)(len - o) : 16u);
    if (!OPEN) {
      uint8_t *tagp = batch_tag(b, rec);
      store_block(tagp, z, M < 16 ? M : 16u);
      if (M > 16) store_block(tagp + 16, z, M < 32 ? M - 16 : 16u);
    }
  }
}

template <bool OPEN, int NR, bool KEYSET>
void launch_one(const CtrHmacKeyDev *keys, const BatchDesc &b, hipStream_t s) {
  unsigned threads = Shape<NR, KEYSET>::kThreads;
  // One key: a batch too small to give every CU a full workgroup takes
  // workgroups of half the size, on twice as many CUs (64K x 16 KiB: 171
  // workgroups instead of 86, 242 GB/s instead of 181).
  if (!KEYSET && b.num_records < (uint64_t)threads * (uint64_t)device_cu_count()) threads /= 2;
  const unsigned grid = (unsigned)((b.num_records + threads - 1) / threads);
  hipLaunchKernelGGL((ctr_hmac_kernel<OPEN, NR, KEYSET>), dim3(grid), dim3(threads), 0, s, keys, b);
}

template <bool OPEN>
void launch_mode(const CtrHmacKeyDev *keys, const BatchDesc &b, int nr, hipStream_t s) {
  const bool keyset = b.key_index != nullptr;
  if (nr == 14)
    keyset ? launch_one<OPEN, 14, true>(keys, b, s) : launch_one<OPEN, 14, false>(keys, b, s);
  else
    keyset ? launch_one<OPEN, 10, true>(keys, b, s) : launch_one<OPEN, 10, false>(keys, b, s);
}

}  // namespace

int launch_ctr_hmac(const CtrHmacKeyDev *keys, const BatchDesc &b, bool open, int nr, void *stream,
                    const KernelEvents *ev) {
  if (b.extra || b.extra_len || b.iovecs) return 1;  // not supported by this AEAD's kernel
  if (nr != 10 && nr != 14) return 1;
  if (b.num_records == 0) return 0;
  if ((b.num_records + 383) / 384 > 0x7fffffffu) return 1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  BatchDesc bo = b;  // with the processing order of a ragged batch
  uint32_t *order = nullptr;
  if (wants_length_order(b)) {
    if (hipMallocAsync(reinterpret_cast<void **>(&order), (b.num_records + 128) * sizeof(uint32_t),
                       s) != hipSuccess)
      return 2;
    const int orc = build_length_order(b.lengths, b.num_records, order, order + b.num_records, s);
    if (orc) {
      hipFreeAsync(order, s);
      return orc;
    }
    bo.order = order;
  }
  if (ev) hipEventRecord(reinterpret_cast<hipEvent_t>(ev->start), s);
  open ? launch_mode<true>(keys, bo, nr, s) : launch_mode<false>(keys, bo, nr, s);
  const int rc = (int)hipGetLastError();
  if (ev) hipEventRecord(reinterpret_cast<hipEvent_t>(ev->stop), s);
  if (order) hipFreeAsync(order, s);
  return rc;
}

}  // namespace bssl_amd
