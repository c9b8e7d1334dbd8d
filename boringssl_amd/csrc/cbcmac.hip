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
// * One key: the round keys are wave-uniform (scalar loads).  Keysets: each
//   lane copies its key's schedule into an LDS slot of its own with an odd
//   stride in words, so the 64 lanes' reads of word w fall in 64 different
//   banks.  The workgroup is as large as 160 KiB of LDS allows next to the
//   64 KiB of tables.
// * Ragged batches are processed in the order of build_length_order, so the
//   lanes of a wave run similar trip counts.
#include <hip/hip_runtime.h>

#include "aes_tables.h"
#include "internal.h"
#include "rec_blocks.h"

namespace bssl_amd {
namespace {

// Threads per workgroup and the LDS slot stride (words) of a lane's round keys.
template <int NR, bool KEYSET>
struct Shape {
  static constexpr int kStride = 4 * (NR + 1) + 1;  // odd: 45 or 61
  static constexpr int kThreads = KEYSET && NR == 14 ? 384 : 512;
  static constexpr int kSlotWords = KEYSET ? kThreads * kStride : 1;
};

template <int NR, bool KEYSET>
struct Lds {
  uint32_t t[256][2][32];  // T0 / T1, replica (lane & 31)
  uint32_t slot[Shape<NR, KEYSET>::kSlotWords];
};
static_assert(sizeof(Lds<10, true>) <= 160 * 1024 && sizeof(Lds<14, true>) <= 160 * 1024 &&
                  sizeof(Lds<10, false>) <= 80 * 1024 && sizeof(Lds<14, false>) <= 80 * 1024,
              "LDS per workgroup (one-key kernels: two workgroups per CU)");
static_assert(Shape<10, true>::kStride % 2 == 1 && Shape<14, true>::kStride % 2 == 1,
              "odd slot stride: lane l's word w in bank (l * stride + w) % 64, all different");

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
__global__ __launch_bounds__((Shape<NR, KEYSET>::kThreads)) void cbcmac_kernel(
    const CbcKeyDev *__restrict__ keys, BatchDesc b) {
  using S = Shape<NR, KEYSET>;
  __shared__ Lds<NR, KEYSET> L;
  for (int e = threadIdx.x; e < 256 * 64; e += S::kThreads) {
    const uint32_t v = kAesTables.te0[e >> 6];
    (&L.t[0][0][0])[e] = ((e >> 5) & 1) ? rotl(v, 8) : v;
  }
  const uint64_t pos = (uint64_t)blockIdx.x * S::kThreads + threadIdx.x;
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
    live = kidx < b.num_keys && meta<uint8_t>(b.valid, rec, 1) != 0;
    // e_aesccm.cc.inc:71-78, 188-191; e_aeseax.cc:76, 234, 276-284.
    if (EAX)
      live = live && b.tag_len == 16 && (b.nonce_len == 12 || b.nonce_len == 16);
    else
      live = live && b.nonce_len == 13 && len <= kCcmMaxInput && b.tag_len >= 4 &&
             b.tag_len <= 16 && (b.tag_len & 1) == 0;
  }
  // Round keys: the key's own (global, wave-uniform) or the lane's LDS slot.
  const CbcKeyDev &K = keys[live ? kidx : 0];
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
  if (!active) return;
  if (b.status) b.status[rec] = ok ? 1 : 0;
  if (!ok) {
    // A failed record's output (and the tag of a failed seal) zero-filled
    // (aead.cc.inc:132-139, 539-547): a second pass over this record only.
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint64_t o = 0; o < len; o += 16) store_block(dst + o, z, len - o < 16 ? (uint32_t)(len - o) : 16u);
    if (!OPEN) store_block(tagp, z, M < 16 ? M : 16u);
  }
}

template <bool EAX, bool OPEN, int NR, bool KEYSET>
void launch_one(const CbcKeyDev *keys, const BatchDesc &b, hipStream_t s) {
  constexpr unsigned threads = Shape<NR, KEYSET>::kThreads;
  const unsigned grid = (unsigned)((b.num_records + threads - 1) / threads);
  hipLaunchKernelGGL((cbcmac_kernel<EAX, OPEN, NR, KEYSET>), dim3(grid), dim3(threads), 0, s, keys,
                     b);
}

template <bool EAX, bool OPEN>
void launch_mode(const CbcKeyDev *keys, const BatchDesc &b, int nr, hipStream_t s) {
  const bool keyset = b.key_index != nullptr;
  if (nr == 14)
    keyset ? launch_one<EAX, OPEN, 14, true>(keys, b, s) : launch_one<EAX, OPEN, 14, false>(keys, b, s);
  else
    keyset ? launch_one<EAX, OPEN, 10, true>(keys, b, s) : launch_one<EAX, OPEN, 10, false>(keys, b, s);
}

}  // namespace

int launch_cbcmac(const CbcKeyDev *keys, const BatchDesc &b, bool eax, bool open, int nr,
                  void *stream, const KernelEvents *ev) {
  if (b.extra || b.extra_len || b.iovecs) return 1;  // not supported by these AEADs' kernel
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
  if (eax)
    open ? launch_mode<true, true>(keys, bo, nr, s) : launch_mode<true, false>(keys, bo, nr, s);
  else
    open ? launch_mode<false, true>(keys, bo, nr, s) : launch_mode<false, false>(keys, bo, nr, s);
  const int rc = (int)hipGetLastError();
  if (ev) hipEventRecord(reinterpret_cast<hipEvent_t>(ev->stop), s);
  if (order) hipFreeAsync(order, s);
  return rc;
}

}  // namespace bssl_amd
