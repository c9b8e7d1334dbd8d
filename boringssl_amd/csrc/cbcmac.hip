// cbcmac.hip -- AES-CCM and AES-EAX seal / open over device-resident record
// batches: the AEADs that pair AES-CTR with a serial AES MAC chain (CBC-MAC
// for CCM, OMAC for EAX).
//
// Replaces aead_aes_ccm_sealv / _openv_detached
// (crypto/fipsmodule/cipher/e_aesccm.cc.inc:312-383, with ccm128_init_state,
// ccm128_encrypt and ccm128_compute_mac, :61-226) and aead_aes_eax_sealv /
// _openv_detached (crypto/cipher/e_aeseax.cc:221-315, with omac_with_tag and
// aes_ctr, :121-219).  Written from RFC 3610 and the EAX paper (Bellare,
// Rogaway, Wagner, FSE 2004).  Design:
// * The MAC chain of a record cannot be split, so records are the unit of
//   parallelism: one lane per record.  Each step of a record's single pass
//   runs two independent AES blocks in the lane -- the chain's next block and
//   a counter block -- round by round, so two lookup chains are in flight.
//   CCM seal and EAX open take both from the block just loaded; CCM open and
//   EAX seal authenticate what the keystream produces, so they run the
//   keystream one block ahead of the chain.
// * AES by the bank-replicated T-tables of aes_tables.h: every lane reads its
//   own bank whatever the (secret) index.
// * The frame around the AEAD -- LDS layout, the lane's record and round keys
//   (wave-uniform for one key, per-lane LDS slots for keysets), the failed
//   record's zero-fill, the launcher with the length order of ragged batches
//   -- is lane_frame.h.
#include <hip/hip_runtime.h>

#include "aes_tables.h"
#include "internal.h"
#include "lane_frame.h"
#include "rec_blocks.h"

namespace bssl_amd {
namespace {

// Threads per workgroup: two workgroups per CU for one key; for keysets as
// many lanes as 160 KiB of LDS hold slots for (lane_frame.h).
constexpr int cbcmac_threads(int nr, bool keyset) { return keyset && nr == 14 ? 384 : 512; }

// ---- the two modes -----------------------------------------------------------

// OMAC's last block (pad, e_aeseax.cc:108-119): a whole block XOR B, a partial
// one (zero-padded here) with 0x80 appended XOR P.
__device__ __forceinline__ uint4 omac_last(uint4 blk, uint32_t n, uint4 B, uint4 P) {
  return n == 16 ? xor4(blk, B) : xor4(or_byte(blk, n, 0x80), P);
}

// N + p on the whole 128-bit big-endian counter (AES_ctr128_encrypt): nbe =
// the counter's big-endian words, most significant first.  One carry chain
// over the four words.
__device__ __forceinline__ uint4 eax_counter(const uint32_t (&nbe)[4], uint64_t p) {
  uint64_t t = (uint64_t)nbe[3] + (uint32_t)p;
  const uint32_t r3 = (uint32_t)t;
  t = (uint64_t)nbe[2] + (uint32_t)(p >> 32) + (t >> 32);
  const uint32_t r2 = (uint32_t)t;
  t = (uint64_t)nbe[1] + (t >> 32);
  const uint32_t r1 = (uint32_t)t;
  t = (uint64_t)nbe[0] + (t >> 32);
  const uint32_t r0 = (uint32_t)t;
  return make_uint4(__builtin_bswap32(r0), __builtin_bswap32(r1), __builtin_bswap32(r2),
                    __builtin_bswap32(r3));
}

// CCM's counter block A_c (RFC 3610 2.3, L = 2): a0 = A_0, c in the last two
// bytes, big-endian.
__device__ __forceinline__ uint4 ccm_counter(uint4 a0, uint32_t c) {
  return make_uint4(a0.x, a0.y, a0.z, a0.w | ((c >> 8) & 0xff) << 16 | (c & 0xff) << 24);
}

// Block j of CCM's encoded AD (RFC 3610 2.2; ccm128_init_state,
// e_aesccm.cc.inc:95-145): the length -- 2 bytes below 0xff00, ff fe and 4
// bytes up to 2^32 - 1, else ff ff and 8 bytes -- then the AD, zero-padded to
// a block boundary.
__device__ __forceinline__ uint4 ccm_ad_block(const uint8_t *ad, uint64_t ad_len, uint64_t j) {
  const uint32_t pre = ad_len < 0xff00 ? 2 : ad_len <= 0xffffffffu ? 6 : 10;
  if (j) {
    const uint64_t o = 16 * j - pre, left = ad_len - o;
    return load_block(ad + o, left < 16 ? (uint32_t)left : 16u);
  }
  uint4 v = make_uint4(0, 0, 0, 0);
  if (pre == 2) {
    v.x = (uint32_t)(ad_len >> 8) | ((uint32_t)ad_len & 0xff) << 8;
  } else if (pre == 6) {
    const uint32_t l = (uint32_t)ad_len;
    v.x = 0xfeffu | (l >> 24) << 16 | ((l >> 16) & 0xff) << 24;
    v.y = ((l >> 8) & 0xff) | (l & 0xff) << 8;
  } else {
    const uint32_t h = (uint32_t)(ad_len >> 32), l = (uint32_t)ad_len;
    v.x = 0xffffu | (h >> 24) << 16 | ((h >> 16) & 0xff) << 24;
    v.y = ((h >> 8) & 0xff) | (h & 0xff) << 8 | (l >> 24) << 16 | ((l >> 16) & 0xff) << 24;
    v.z = ((l >> 8) & 0xff) | (l & 0xff) << 8;
  }
  for (uint32_t i = pre; i < 16 && i - pre < ad_len; i++) v = or_byte(v, i, ad[i - pre]);
  return v;
}

// One record per lane.  EAX: AES-EAX, else AES-CCM with L = 2 and M =
// b.tag_len.
template <bool EAX, bool OPEN, int NR, bool KEYSET>
__global__ __launch_bounds__((cbcmac_threads(NR, KEYSET))) void cbcmac_kernel(
    const CbcKeyDev *__restrict__ keys, BatchDesc b) {
  constexpr int kThreads = cbcmac_threads(NR, KEYSET);
  __shared__ LaneLds<NR, KEYSET, kThreads> L;
  lane_fill_tables(L, kAesTables.te0, kThreads);
  const LaneRecord r = lane_record<KEYSET>(b, kThreads);
  const bool active = r.active;
  const uint64_t rec = r.rec, off = r.off, len = r.len, ad_off = r.ad_off, ad_len = r.ad_len;
  bool live = r.live;
  if (active) {
    // e_aesccm.cc.inc:71-78, 188-191; e_aeseax.cc:76, 234, 276-284.
    if (EAX)
      live = live && b.tag_len == 16 && (b.nonce_len == 12 || b.nonce_len == 16);
    else
      live = live && b.nonce_len == 13 && len <= kCcmMaxInput && b.tag_len >= 4 &&
             b.tag_len <= 16 && (b.tag_len & 1) == 0;
  }
  const CbcKeyDev &K = keys[live ? r.kidx : 0];
  const uint32_t *rk = lane_round_keys<NR, KEYSET>(&K.rk[0][0], L);

  const uint32_t M = b.tag_len;
  const uint8_t *src = b.in + off;
  uint8_t *dst = b.out + off;
  uint8_t *tagp = active ? batch_tag(b, rec) : nullptr;
  int ok = live;
  if (live) {
    const uint8_t *ad = b.ad + ad_off;
    const uint64_t nb = (len + 15) / 16;
    const uint4 nw = load_block(b.nonces + rec * b.nonce_len, (uint32_t)b.nonce_len);
    uint4 B = make_uint4(0, 0, 0, 0), P = B, a0 = B;
    uint64_t nA;  // blocks of the AD chain
    uint4 s[2];
    if constexpr (EAX) {
      B = make_uint4(K.eax_b[0], K.eax_b[1], K.eax_b[2], K.eax_b[3]);
      P = make_uint4(K.eax_p[0], K.eax_p[1], K.eax_p[2], K.eax_p[3]);
      // N = OMAC^0(nonce) and the first step of H = OMAC^1(AD): the chains
      // start from E_K(0^15 || t); an empty input is E_K((0^15 || t) ^ B).
      nA = (ad_len + 15) / 16;
      s[0] = xor4(make_uint4(K.eax_e[0][0], K.eax_e[0][1], K.eax_e[0][2], K.eax_e[0][3]),
                  omac_last(nw, (uint32_t)b.nonce_len, B, P));
      if (nA == 0) {
        s[1] = make_uint4(B.x, B.y, B.z, B.w ^ 0x01000000u);
      } else {
        const uint32_t n0 = ad_len < 16 ? (uint32_t)ad_len : 16u;
        const uint4 blk = load_block(ad, n0);
        s[1] = xor4(make_uint4(K.eax_e[1][0], K.eax_e[1][1], K.eax_e[1][2], K.eax_e[1][3]),
                    nA == 1 ? omac_last(blk, n0, B, P) : blk);
      }
    } else {
      // B_0 = flags || nonce || len and A_0 = (L - 1) || nonce || 0 (RFC 3610
      // 2.2, 2.3; e_aesccm.cc.inc:82-92, 161).
      const uint32_t pre = ad_len < 0xff00 ? 2 : ad_len <= 0xffffffffu ? 6 : 10;
      nA = ad_len ? (ad_len + pre + 15) / 16 : 0;
      const uint32_t flags = 1u | ((M - 2) / 2) << 3 | (ad_len ? 0x40u : 0u);
      a0 = make_uint4((nw.x << 8) | 1u, (nw.y << 8) | (nw.x >> 24), (nw.z << 8) | (nw.y >> 24),
                      (nw.w << 8) | (nw.z >> 24));
      s[0] = make_uint4((a0.x & ~0xffu) | flags, a0.y, a0.z,
                        a0.w | (((uint32_t)len >> 8) & 0xff) << 16 | ((uint32_t)len & 0xff) << 24);
      s[1] = a0;
    }
    aes_n<NR, 2>(s, rk, L);
    // The AD chain: CCM's CBC-MAC goes on into the message; EAX's H.
    uint4 chain = EAX ? s[1] : s[0];
    const uint4 first = EAX ? s[0] : s[1];  // EAX: N; CCM: E_K(A_0)
    for (uint64_t j = EAX ? 1 : 0; j < nA; j++) {
      uint4 blk;
      if constexpr (EAX) {
        const uint64_t left = ad_len - 16 * j;
        const uint32_t n = left < 16 ? (uint32_t)left : 16u;
        blk = load_block(ad + 16 * j, n);
        if (j + 1 == nA) blk = omac_last(blk, n, B, P);
      } else {
        blk = ccm_ad_block(ad, ad_len, j);
      }
      uint4 one[1] = {xor4(chain, blk)};
      aes_n<NR, 1>(one, rk, L);
      chain = one[0];
    }
    uint32_t nbe[4] = {0, 0, 0, 0};
    if constexpr (EAX) {
      nbe[0] = __builtin_bswap32(first.x);
      nbe[1] = __builtin_bswap32(first.y);
      nbe[2] = __builtin_bswap32(first.z);
      nbe[3] = __builtin_bswap32(first.w);
    }
    // Counter block of message block p (CCM's data counters start at 1).
    auto counter = [&](uint64_t p) {
      if constexpr (EAX) return eax_counter(nbe, p);
      else return ccm_counter(a0, (uint32_t)p + 1);
    };
    // The chain through the message: CCM's X goes on from the AD; EAX's
    // C = OMAC^2(ciphertext) starts at E_K(0^15 || 2).  DEP: the chain takes
    // what the keystream produces (CCM open: the plaintext, EAX seal: the
    // ciphertext), so the keystream runs one block ahead of it.
    constexpr bool DEP = EAX != OPEN;
    uint4 X = chain, ks = make_uint4(0, 0, 0, 0);
    if constexpr (EAX) X = make_uint4(K.eax_e[2][0], K.eax_e[2][1], K.eax_e[2][2], K.eax_e[2][3]);
    if (DEP || (EAX && nb == 0)) {
      s[0] = make_uint4(B.x, B.y, B.z, B.w ^ 0x02000000u);  // EAX, empty message: C
      s[1] = counter(0);
      aes_n<NR, 2>(s, rk, L);
      if (EAX && nb == 0) X = s[0];
      ks = s[1];
    }
    for (uint64_t p = 0; p < nb; p++) {
      const uint64_t left = len - 16 * p;
      const uint32_t n = left < 16 ? (uint32_t)left : 16u;
      const uint4 x = load_block(src + 16 * p, n);
      uint4 y = x;
      if constexpr (DEP) {
        y = mask_block(xor4(x, ks), n);
        store_block(dst + 16 * p, y, n);
      }
      // The chain's input: the plaintext for CCM (zero-padded), the
      // ciphertext for EAX (OMAC-padded at the end).
      uint4 m = y;
      if (EAX && p + 1 == nb) m = omac_last(m, n, B, P);
      s[0] = xor4(X, m);
      s[1] = counter(DEP ? p + 1 : p);
      aes_n<NR, 2>(s, rk, L);
      X = s[0];
      if constexpr (DEP)
        ks = s[1];
      else
        store_block(dst + 16 * p, xor4(x, s[1]), n);
    }
    // CCM: the MAC encrypted with counter 0, first M bytes.  EAX: N ^ H ^ C.
    uint4 tag = xor4(X, first);
    if constexpr (EAX) tag = xor4(tag, chain);
    tag = mask_block(tag, M);
    if constexpr (OPEN) {
      // All M bytes compared, no early exit (CRYPTO_memcmp).
      const uint4 t = mask_block(load_block(tagp, M), M);
      ok = ((t.x ^ tag.x) | (t.y ^ tag.y) | (t.z ^ tag.z) | (t.w ^ tag.w)) == 0;
    } else {
      store_block(tagp, tag, M);
    }
  }
  if (active) lane_finish<OPEN>(b, rec, ok, len, dst, M < 16 ? M : 16u);
}

}  // namespace

int launch_cbcmac(const CbcKeyDev *keys, const BatchDesc &b, bool eax, bool open, int nr,
                  void *stream, const KernelEvents *ev) {
  const bool keyset = b.key_index != nullptr;
  return launch_lane_kernel(
      b, nr == 10 || nr == 14, cbcmac_threads(nr, keyset), /*half_rule=*/false, stream, ev,
      [&](const BatchDesc &bo, unsigned grid, unsigned threads, hipStream_t s) {
        with_nr_keyset(nr, keyset, [&](auto NR, auto KEYSET) {
          auto go = [&](auto EAX, auto OPEN) {
            hipLaunchKernelGGL((cbcmac_kernel<EAX.value, OPEN.value, NR.value, KEYSET.value>),
                               dim3(grid), dim3(threads), 0, s, keys, bo);
          };
          if (eax)
            open ? go(std::true_type{}, std::true_type{}) : go(std::true_type{}, std::false_type{});
          else
            open ? go(std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{});
        });
      });
}

}  // namespace bssl_amd
