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
//   parallelism: one lane per record, in the frame of lane_frame.h (DESIGN.md
//   4.11a): LDS layout, the lane's record and round keys, the failed record's
//   zero-fill, the launcher with the length order of ragged batches.
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
//   loads).  Keysets: round keys in the frame's per-lane LDS slots; the two
//   states are read from global memory once each.
#include <hip/hip_runtime.h>

#include "aes_tables.h"
#include "internal.h"
#include "lane_frame.h"
#include "rec_blocks.h"
#include "sha_compress.h"

namespace bssl_amd {
namespace {

// Threads per workgroup.  One key: the kernels take 144 VGPRs, three waves per
// SIMD, and a CU takes them as one workgroup of twelve waves (the dispatcher
// placed no second workgroup of six waves beside the first: 1.5 waves per SIMD
// measured).  This is the largest workgroup; small one-key batches take half
// (launch_lane_kernel's half_rule), so the kernel reads blockDim.x.
// Keysets: as large as 160 KiB of LDS allows.
constexpr int ctr_hmac_threads(int nr, bool keyset) { return !keyset ? 768 : nr == 14 ? 384 : 512; }

// One record per lane.
template <bool OPEN, int NR, bool KEYSET>
__global__ __launch_bounds__((ctr_hmac_threads(NR, KEYSET))) void ctr_hmac_kernel(
    const AesHmacKeyDev *__restrict__ keys, BatchDesc b) {
  __shared__ LaneLds<NR, KEYSET, ctr_hmac_threads(NR, KEYSET)> L;
  lane_fill_tables(L, kAesTables.te0, blockDim.x);
  const LaneRecord r = lane_record<KEYSET>(b, blockDim.x);
  const bool active = r.active;
  const uint64_t rec = r.rec, off = r.off, len = r.len, ad_off = r.ad_off, ad_len = r.ad_len;
  bool live = r.live;
  // e_aesctrhmac.cc:97, 190, 201, 226, 237.  A record of 2^36 bytes or more
  // (the 32-bit block counter would wrap) fails alone, status 0, as gcm.hip
  // treats its own limit; no test can allocate one.
  if (active) live = live && b.nonce_len == 12 && b.tag_len <= 32 && len <= kCtrHmacMaxInput;
  const AesHmacKeyDev &K = keys[live ? r.kidx : 0];
  const uint32_t *rk = lane_round_keys<NR, KEYSET>(&K.rk[0][0], L);

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
        // SHA's padding; the ipad block counts in the length.
        sha_padding(w, len, base, q + 1 == nM, 8 * (64 + 64 * nH + len));
      } else {
        // The outer hash: one block, the inner digest with its padding, from
        // the state after the opad block.
        hmac_outer_block<8>(h, w);
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = K.outer[i];
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
  if (active) lane_finish<OPEN>(b, rec, ok, len, dst, M < 32 ? M : 32u);
}

}  // namespace

int launch_ctr_hmac(const AesHmacKeyDev *keys, const BatchDesc &b, bool open, int nr, void *stream,
                    const KernelEvents *ev) {
  const bool keyset = b.key_index != nullptr;
  return launch_lane_kernel(
      b, nr == 10 || nr == 14, ctr_hmac_threads(nr, keyset), /*half_rule=*/true, stream, ev,
      [&](const BatchDesc &bo, unsigned grid, unsigned threads, hipStream_t s) {
        with_nr_keyset(nr, keyset, [&](auto NR, auto KEYSET) {
          if (open)
            hipLaunchKernelGGL((ctr_hmac_kernel<true, NR.value, KEYSET.value>), dim3(grid),
                               dim3(threads), 0, s, keys, bo);
          else
            hipLaunchKernelGGL((ctr_hmac_kernel<false, NR.value, KEYSET.value>), dim3(grid),
                               dim3(threads), 0, s, keys, bo);
        });
      });
}

}  // namespace bssl_amd
