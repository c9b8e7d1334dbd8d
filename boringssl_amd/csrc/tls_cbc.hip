// tls_cbc.hip -- the TLS 1.1 / 1.2 MAC-then-encrypt AEADs with an explicit IV
// (AES-128/256-CBC with HMAC-SHA1, AES-128-CBC with HMAC-SHA256) over
// device-resident record batches.
//
// Replaces aead_tls_sealv / aead_tls_openv (crypto/cipher/e_tls.cc:118-410)
// and, for open, EVP_tls_cbc_remove_padding, EVP_tls_cbc_copy_mac and
// EVP_tls_cbc_digest_record (crypto/cipher/tls_cbc.cc).  Written from FIPS 197
// (the cipher and 5.3.5's equivalent inverse cipher), FIPS 180-4, RFC 2104 and
// RFC 5246 6.2.3.2, whose construction those files implement:
//   mac  = HMAC(mac key, ad (11 bytes) || be16(len) || plaintext)
//   wire = AES-CBC(iv = nonce, plaintext || mac || pad_len x byte(pad_len - 1)),
//          pad_len = 16 - (len + mac_len) % 16
// Seal writes wire[0, len) to the record and the rest (the "tag", mac_len +
// pad_len bytes) to the record's tag slot; open takes the whole wire.
// Design:
// * Neither the CBC-encrypt chain nor the hash chain of a record can be
//   split: one lane per record, in the frame of lane_frame.h (DESIGN.md
//   4.11a): LDS layout, the lane's record and round keys, the failed record's
//   zero-fill, the launcher with the length order of ragged batches.
// * One loop per record over the 64-byte blocks of the hash.  The hash stream
//   is 13 bytes ahead of the record's 16-byte blocks; a step builds its hash
//   block from the previous step's last record block (kept in registers) and
//   its own four (v_alignbyte), never reading a byte twice.
// * Seal: the steps whose four record blocks are whole run the four chained
//   AES blocks (LDS lookups, rounds unrolled) and the compression (VALU) with
//   no condition between them; the steps at the record's end take a general
//   path.  The tail (plaintext remainder, MAC, padding) goes through the same
//   chain.  (The two are independent and written back to back, but the
//   compiler does not interleave them: DESIGN.md 4.14.)
// * Open: the last block is decrypted first for the padding byte; then one
//   pass, four blocks through the inverse cipher together (aes_dec_n).  What
//   depends on the padding byte is done by masks only -- see "constant shape"
//   at tls_cbc_kernel.
// * One key: the round keys and both HMAC states are wave-uniform.  Keysets:
//   round keys in the frame's per-lane LDS slots.
#include <hip/hip_runtime.h>

#include "aes_inv_tables.h"
#include "aes_tables.h"
#include "internal.h"
#include "lane_frame.h"
#include "rec_blocks.h"
#include "sha_compress.h"

namespace bssl_amd {
namespace {

// Threads per workgroup (the largest: small one-key batches take half,
// launch_lane_kernel's half_rule, so the kernel reads blockDim.x).  One key:
// the AES-128 seal kernels take at most 128 VGPRs, four waves per SIMD as two
// workgroups of eight waves; the others (131 to 156 VGPRs) three, as one
// workgroup of twelve.  Keysets: as large as 160 KiB of LDS allows.
constexpr int tls_cbc_threads(bool open, int nr, bool keyset) {
  return !keyset ? (open || nr == 14 ? 768 : 512) : nr == 14 ? 384 : 512;
}

template <bool SHA1>
struct Mac {
  static constexpr uint32_t kLen = SHA1 ? 20 : 32;  // the MAC
  static constexpr int kWords = kLen / 4;
  static constexpr uint32_t kSlot = kLen + 16;      // the tag slot: MAC and the longest padding
  static __device__ __forceinline__ void compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
    if constexpr (SHA1) sha1_compress(h, w); else sha256_compress(h, w);
  }
};

// One block through the cipher; FLAT: the rounds unrolled, else a loop.
template <int NR, bool FLAT, class LDS>
__device__ __forceinline__ uint4 aes_block(uint4 v, const uint32_t *rk, const LDS &L) {
  if constexpr (!FLAT) {
    uint4 s[1] = {v};
    aes_n<NR, 1>(s, rk, L);
    return s[0];
  } else {
    uint32_t s0 = v.x ^ rk[0], s1 = v.y ^ rk[1], s2 = v.z ^ rk[2], s3 = v.w ^ rk[3];
#pragma unroll
    for (int r = 1; r < NR; r++) {
      auto col = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t kk) {
        return t0(L, a & 0xff) ^ t1(L, (b >> 8) & 0xff) ^
               rotl(t0(L, (c >> 16) & 0xff) ^ t1(L, d >> 24), 16) ^ kk;
      };
      const uint32_t n0 = col(s0, s1, s2, s3, rk[4 * r]), n1 = col(s1, s2, s3, s0, rk[4 * r + 1]),
                     n2 = col(s2, s3, s0, s1, rk[4 * r + 2]), n3 = col(s3, s0, s1, s2, rk[4 * r + 3]);
      s0 = n0; s1 = n1; s2 = n2; s3 = n3;
    }
    auto last = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
      return sbox(L, a & 0xff) | (sbox(L, (b >> 8) & 0xff) << 8) |
             (sbox(L, (c >> 16) & 0xff) << 16) | (sbox(L, d >> 24) << 24);
    };
    return make_uint4(last(s0, s1, s2, s3) ^ rk[4 * NR], last(s1, s2, s3, s0) ^ rk[4 * NR + 1],
                      last(s2, s3, s0, s1) ^ rk[4 * NR + 2], last(s3, s0, s1, s2) ^ rk[4 * NR + 3]);
  }
}

// x := the bytes of x from byte offset n on, zeros past the end; n <= MAXN.
// Selects only: no branch and no address depends on n.
template <int MAXN, int N>
__device__ __forceinline__ void take_from(uint32_t (&x)[N], uint32_t n) {
  const uint32_t bs = n & 3, nw = n >> 2;
#pragma unroll
  for (int i = 0; i < N; i++) x[i] = __builtin_amdgcn_alignbyte(i + 1 < N ? x[i + 1] : 0u, x[i], bs);
#pragma unroll
  for (int bit = 1; 4 * bit <= MAXN; bit <<= 1) {
    const uint32_t m = 0u - ((nw / bit) & 1u);
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = bfi(m, i + bit < N ? x[i + bit] : 0u, x[i]);
  }
}

// All ones where a signed value is negative.
__device__ __forceinline__ uint32_t neg_mask(int32_t v) { return (uint32_t)(v >> 31); }
// min(max(v, lo), hi).
__device__ __forceinline__ int32_t clamp(int32_t v, int32_t lo, int32_t hi) {
  return min(max(v, lo), hi);
}
// The low n bytes of a word set, n clamped to 0..4 (no branch on n).
__device__ __forceinline__ uint32_t low_bytes(int32_t n) {
  return (uint32_t)((uint64_t(1) << (8 * clamp(n, 0, 4))) - 1);
}

// The hash block of a step: the last 13 bytes of `carry`, the blocks v[0..2]
// and the first three bytes of v[3], as sixteen big-endian words.
__device__ __forceinline__ void hash_block(uint4 carry, const uint4 (&v)[4], uint32_t (&w)[16]) {
  const uint32_t f[17] = {carry.x, carry.y, carry.z, carry.w, v[0].x, v[0].y, v[0].z, v[0].w, v[1].x,
                          v[1].y,  v[1].z,  v[1].w,  v[2].x,  v[2].y, v[2].z, v[2].w, v[3].x};
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = __builtin_bswap32(__builtin_amdgcn_alignbyte(f[i + 1], f[i], 3));
}

// One record per lane.
//
// Constant shape of OPEN (Lucky 13): every trip count, every
// branch before the final status write and every global or LDS address is a
// function of public values only -- the record's length, the MAC size, the
// batch layout -- with the table lookups' bank argument of aes_inv_tables.h.
// The padding byte p, data_len and the two verdicts enter selects, masks and
// shift amounts of VALU instructions only.  Names below: `len`, `nblk`, `kh`,
// `kmin`, `jtrail`, `dist*` and `cap` (the record layer's plaintext limit) are
// public; `p`, `padlen`, `dlen`, `bad`, `macacc`, `dig`, `over` are not.
template <bool OPEN, int NR, bool SHA1, bool KEYSET>
__global__ __launch_bounds__((tls_cbc_threads(OPEN, NR, KEYSET))) void tls_cbc_kernel(
    const AesHmacKeyDev *__restrict__ keys, BatchDesc b) {
  using H = Mac<SHA1>;
  constexpr uint32_t M = H::kLen;
  // T0 / T1 (seal) or Td0 / Td1 (open).
  __shared__ LaneLds<NR, KEYSET, tls_cbc_threads(OPEN, NR, KEYSET)> L;
  lane_fill_tables(L, OPEN ? kAesInvTables.td0 : kAesTables.te0, blockDim.x);
  const LaneRecord r = lane_record<KEYSET>(b, blockDim.x);
  const bool active = r.active;
  const uint64_t rec = r.rec, off = r.off, len = r.len, ad_off = r.ad_off, ad_len = r.ad_len;
  // e_tls.cc:137-146, 281-295; open: a length that is no multiple of the
  // block or below the MAC and the padding length byte (:315-319,
  // tls_cbc.cc:37-39).
  bool live = r.live;
  if (active) {
    live = live && b.nonce_len == 16 && ad_len == 11 && b.tag_len == H::kSlot;
    if (OPEN) live = live && (len & 15) == 0 && len >= M + 1;
  }
  const AesHmacKeyDev &K = keys[live ? r.kidx : 0];
  const uint32_t *rk = lane_round_keys<NR, KEYSET>(&K.rk[0][0], L);

  const uint8_t *src = b.in + off;
  uint8_t *dst = b.out + off;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  int ok = live;
  uint64_t dlen = 0;  // open: the plaintext length
  if (live) {
    const uint4 iv = load_block(b.nonces + rec * 16, 16);
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = K.inner[i];
    // The outer hash's block: the inner digest with SHA's padding; h restarts
    // from the state after the opad block.
    auto outer_block = [&](const uint32_t (&inner)[8], uint32_t (&w)[16]) {
      hmac_outer_block<H::kWords>(inner, w);
#pragma unroll
      for (int i = 0; i < 8; i++) h[i] = K.outer[i];
    };
    // The 13 bytes before the plaintext in the hash stream, as the last 13
    // bytes of a block: ad || be16(length).
    auto header = [&](uint32_t len16) {
      const uint4 a = load_block(b.ad + ad_off, 11);
      return make_uint4(a.x << 24, __builtin_amdgcn_alignbyte(a.y, a.x, 1),
                        __builtin_amdgcn_alignbyte(a.z, a.y, 1),
                        ((a.z >> 8) & 0xffffu) | ((len16 >> 8) << 16) | ((len16 & 0xffu) << 24));
    };

    if constexpr (!OPEN) {
      // The length as 16 bits, wrapping (e_tls.cc:151).
      uint4 carry = header((uint32_t)len & 0xffffu);
      const uint64_t hlen = 13 + len;  // the inner hash's message after the ipad block
      const uint64_t nM = hlen / 64 + 1 + ((hlen & 63) >= 56 ? 1 : 0);
      const uint64_t bits = 8 * (64 + hlen);
      const uint64_t nfull = len / 64;  // steps whose four record blocks are whole
      uint4 c = iv, rem = zero;
      for (uint64_t t = 0; t <= nM; t++) {
        uint32_t w[16];
        if (t < nfull) {
          // (hlen - 64 t >= 64 + 13: no SHA padding in this block.)
          const uint8_t *p = src + 64 * t;
          uint8_t *q = dst + 64 * t;
          uint4 v[4];
#pragma unroll
          for (int k = 0; k < 4; k++) v[k] = load_block(p + 16 * k, 16);
          hash_block(carry, v, w);
          carry = v[3];
          // The chain (LDS lookups, serial) and the compression (VALU) are
          // independent.  (The compiler sinks the compression below the
          // stores' alignment branches; pinning it here cost the fourth wave
          // per SIMD)
#pragma unroll
          for (int k = 0; k < 4; k++) v[k] = c = aes_block<NR, true>(xor4(v[k], c), rk, L);
          H::compress(h, w);
#pragma unroll
          for (int k = 0; k < 4; k++) store_block(q + 16 * k, v[k], 16);
          continue;
        }
        if (t < nM) {
          const uint64_t base = 64 * t;
          uint4 v[4];
          uint32_t n[4];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            n[k] = span16(len, base + 16 * k);
            v[k] = n[k] ? load_block(src + base + 16 * k, n[k]) : zero;
          }
          hash_block(carry, v, w);
          carry = v[3];
          sha_padding(w, hlen, base, t + 1 == nM, bits);
          // The whole blocks through the chain; the partial one waits for the MAC.
#pragma unroll
          for (int k = 0; k < 4; k++) {
            if (n[k] == 16) {
              c = aes_block<NR, false>(xor4(v[k], c), rk, L);
              store_block(dst + base + 16 * k, c, 16);
            } else if (n[k]) {
              rem = v[k];
            }
          }
        } else {
          uint32_t inner[8];
#pragma unroll
          for (int i = 0; i < 8; i++) inner[i] = h[i];
          outer_block(inner, w);
        }
        H::compress(h, w);
      }
      // The tail: remainder (r bytes) || mac || padding, 2 to 4 blocks.
      const uint32_t r = (uint32_t)len & 15;
      const uint32_t pad_len = 16 - (((uint32_t)len + M) & 15);
      const uint32_t nT = (r + M + pad_len) / 16;
      uint32_t x[20];
#pragma unroll
      for (int i = 0; i < 20; i++)
        x[i] = i < 4 ? 0u : i < 4 + H::kWords ? __builtin_bswap32(h[i - 4]) : (pad_len - 1) * 0x01010101u;
      take_from<16>(x, 16 - r);
      x[0] |= rem.x; x[1] |= rem.y; x[2] |= rem.z; x[3] |= rem.w;
      uint32_t e[16];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        uint4 y = zero;
        if ((uint32_t)i < nT)
          y = c = aes_block<NR, false>(xor4(make_uint4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]), c), rk, L);
        e[4 * i] = y.x; e[4 * i + 1] = y.y; e[4 * i + 2] = y.z; e[4 * i + 3] = y.w;
      }
      // The first r bytes end the record; what follows (mac_len + pad_len
      // bytes) is the tag, and the rest of its slot is zero.
      if (r) store_block(dst + (len - r), make_uint4(e[0], e[1], e[2], e[3]), r);
      take_from<16>(e, r);
      uint8_t *tagp = batch_tag(b, rec);
#pragma unroll
      for (uint32_t i = 0; 16 * i < H::kSlot; i++)
        store_block(tagp + 16 * i, make_uint4(e[4 * i], e[4 * i + 1], e[4 * i + 2], e[4 * i + 3]),
                    H::kSlot - 16 * i < 16 ? H::kSlot - 16 * i : 16u);
    } else {
      const uint64_t nblk = len / 16;
      // The padding length byte: the last block needs the block before it (or
      // the IV) only.
      uint32_t p;
      {
        uint4 s[1] = {load_block(src + len - 16, 16)};
        const uint4 prev = nblk >= 2 ? load_block(src + len - 32, 16) : iv;
        aes_dec_n<NR, 1>(s, rk, L);
        p = (s[0].w ^ prev.w) >> 24;
      }
      // tls_cbc.cc:43, 73-78: the padding (p + 1 bytes) must leave room for
      // the MAC.  Where it does not, the record fails below; the length goes on
      // as if the padding were its length byte alone, so that dlen stays within
      // what the loop covers.  (The reference takes 0 there and for a wrong
      // padding byte; either way the record fails, and only by `ok`.)
      const uint32_t fits = ~neg_mask((int32_t)(len > 512 ? 512 : (uint32_t)len) - (int32_t)(M + 1 + p));
      const uint32_t padlen = 1 + (p & fits);
      dlen = len - M - padlen;
      // Hash blocks: through the one that ends the longest message possible
      // (padlen 1); masks from the first that may end the shortest (padlen 256).
      const uint64_t kh = (13 + (len - M - 1) + 8) / 64 + 1;
      const uint64_t kmin = len > M + 256 ? (13 + (len - M - 256)) / 64 : 0;
      // Record blocks that may hold padding or MAC bytes: the last 256 + M bytes.
      const uint64_t jtrail = len > M + 256 ? (len - M - 256) / 16 : 0;
      uint4 carry = header((uint32_t)dlen & 0xffffu);
      const uint64_t bits = 8 * (64 + 13 + dlen);
      uint4 cprev = iv;
      uint32_t bad = 0, dig[8] = {0, 0, 0, 0, 0, 0, 0, 0}, macacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (uint64_t t = 0; t <= kh; t++) {
        uint32_t w[16];
        if (t < kh) {
          uint4 ct[4], pt[4];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            ct[k] = 4 * t + k < nblk ? load_block(src + 64 * t + 16 * k, 16) : zero;
            pt[k] = ct[k];
          }
          if (4 * t < nblk) aes_dec_n<NR, 4>(pt, rk, L);
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const uint64_t j = 4 * t + k;
            pt[k] = j < nblk ? xor4(pt[k], k ? ct[k - 1] : cprev) : zero;
            if (j < nblk) store_block(dst + 16 * j, pt[k], 16);
            if (j < nblk && j >= jtrail) {
              // dist: from this block's first byte to the record's end,
              // at most 256 + M + 15.
              const int32_t dist = (int32_t)(len - 16 * j);
              // tls_cbc.cc:58-67: the last p + 1 bytes all equal p -- here the
              // block's bytes from dist - 1 - p on.
              const int32_t keep = dist - 1 - (int32_t)p;
              const uint32_t pp = p * 0x01010101u;
              bad |= ((pt[k].x ^ pp) & ~low_bytes(keep)) | ((pt[k].y ^ pp) & ~low_bytes(keep - 4)) |
                     ((pt[k].z ^ pp) & ~low_bytes(keep - 8)) | ((pt[k].w ^ pp) & ~low_bytes(keep - 12));
              // The record's MAC starts `at` bytes into this block (negative:
              // before it): MAC byte m is this block's byte m + at.
              const int32_t at = dist - (int32_t)(M + padlen);
              uint32_t x[20];
#pragma unroll
              for (int i = 0; i < 20; i++) x[i] = 0;
              x[8] = pt[k].x; x[9] = pt[k].y; x[10] = pt[k].z; x[11] = pt[k].w;
              take_from<48>(x, (uint32_t)clamp(32 + at, 0, 48));
#pragma unroll
              for (int i = 0; i < H::kWords; i++) macacc[i] |= x[i];
            }
          }
          cprev = ct[3];
          hash_block(carry, pt, w);
          carry = pt[3];
          if (t >= kmin) {
            // The message's end relative to this hash block: 0x80 there, zeros
            // after, and the bit length where the block is the message's last.
            const int32_t end = 13 + (int32_t)(int64_t)(len - 64 * t) - (int32_t)(M + padlen);
#pragma unroll
            for (int i = 0; i < 16; i++) {
              const int32_t d = end - 4 * i;  // bytes of word i inside the message
              const uint32_t keepw = ~(uint32_t)(0xffffffffull >> (8 * clamp(d, 0, 4)));
              const uint32_t mark = (uint32_t)((0x80ull << 32) >> (8 * (clamp(d, -1, 4) + 1)));
              w[i] = (w[i] & keepw) | mark;
            }
            const uint32_t is_last = ~neg_mask(end + 8) & neg_mask(end + 8 - 64);
            w[14] |= (uint32_t)(bits >> 32) & is_last;
            w[15] |= (uint32_t)bits & is_last;
            H::compress(h, w);
#pragma unroll
            for (int i = 0; i < 8; i++) dig[i] = bfi(is_last, h[i], dig[i]);
            continue;
          }
        } else {
          outer_block(dig, w);
        }
        H::compress(h, w);
      }
      // The MAC compared in full (CRYPTO_memcmp), and the one verdict.
      uint32_t diff = 0;
#pragma unroll
      for (int i = 0; i < H::kWords; i++) diff |= __builtin_bswap32(h[i]) ^ macacc[i];
      // The record layer's plaintext limit (tls_record.cc:204-209): all ones
      // where dlen exceeds it, one more term of the verdict.
      const uint64_t cap = b.max_plain_len ? b.max_plain_len : ~uint64_t(0) >> 1;
      const uint32_t over = (uint32_t)((int64_t)(cap - dlen) >> 63);
      ok = (diff | bad | ~fits | over) == 0;
    }
  }
  if (!active) return;
  if (OPEN && b.out_lengths) b.out_lengths[rec] = ok ? dlen : 0;
  lane_finish<OPEN>(b, rec, ok, len, dst, H::kSlot);
}

}  // namespace

int launch_tls_cbc(const AesHmacKeyDev *keys, const BatchDesc &b, bool sha1, bool open, int nr,
                   void *stream, const KernelEvents *ev) {
  const bool keyset = b.key_index != nullptr;
  // (AES-256 comes with SHA-1 only.)
  return launch_lane_kernel(
      b, nr == 10 || (nr == 14 && sha1), tls_cbc_threads(open, nr, keyset), /*half_rule=*/true,
      stream, ev, [&](const BatchDesc &bo, unsigned grid, unsigned threads, hipStream_t s) {
        with_nr_keyset(nr, keyset, [&](auto NR, auto KEYSET) {
          auto go = [&](auto OPEN, auto SHA1) {
            if constexpr (NR.value == 10 || SHA1.value)
              hipLaunchKernelGGL((tls_cbc_kernel<OPEN.value, NR.value, SHA1.value, KEYSET.value>),
                                 dim3(grid), dim3(threads), 0, s, keys, bo);
          };
          if (open)
            sha1 ? go(std::true_type{}, std::true_type{}) : go(std::true_type{}, std::false_type{});
          else
            sha1 ? go(std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{});
        });
      });
}

}  // namespace bssl_amd
