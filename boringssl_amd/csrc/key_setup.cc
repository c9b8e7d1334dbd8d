// key_setup.cc -- per-key setup, the analogue of the reference's
// CRYPTO_gcm128_init_aes_key (crypto/fipsmodule/aes/gcm.cc.inc:253-296): the
// tables of key_sched.h built on the host for one key (EVP_AEAD_CTX_init) and
// by a device kernel, one lane per key, for keysets (BSSL_AMD_KEYSET_new:
// 64K keys of config 5 in about a millisecond instead of seconds of host
// work and a host-to-device copy of 12,816 B per key).  Both run the same
// code, so their tables are the same bytes (tests/test_key_setup.py).
#include <string.h>

#include "key_sched.h"
#include "sha256_k.h"

namespace bssl_amd {

void secure_zero(void *p, size_t n) {
  if (n) explicit_bzero(p, n);
}

bool gcm_key_setup(const uint8_t *key, size_t key_len, GcmKeyDev *out) {
  if (key_len != 16 && key_len != 24 && key_len != 32) return false;
  return gcm_key_tables(key, (int)key_len, out);
}

namespace {

// The block times x in GF(2^128) as EAX / OMAC order it (the 16 bytes as one
// big-endian integer, reduced by 0x87; mult_by_X, e_aeseax.cc:50-61), on
// little-endian words of the bytes.  No branch on the (secret) top bit.
void eax_dbl(const uint32_t in[4], uint32_t out[4]) {
  uint32_t be[4];
  for (int i = 0; i < 4; i++) be[i] = ks_bswap(in[i]);
  const uint32_t carry = 0u - (be[0] >> 31);
  for (int i = 0; i < 3; i++) be[i] = (be[i] << 1) | (be[i + 1] >> 31);
  be[3] = (be[3] << 1) ^ (carry & 0x87u);
  for (int i = 0; i < 4; i++) out[i] = ks_bswap(be[i]);
  secure_zero(be, sizeof(be));
}

// The key's FIPS-197 schedule into rk (60 words, which the caller wipes) and,
// as little-endian words, unrotated, into the zeroed *out with its nr.
// Returns nr, or 0 for a bad key length (*out untouched).
template <class KeyDev>
int expand_into(const uint8_t *key, size_t key_len, uint32_t (&rk)[60], KeyDev *out) {
  const int nr = ks_expand(key, (int)key_len, rk);
  if (!nr) return 0;
  memset(out, 0, sizeof(*out));
  for (int r = 0; r <= nr; r++)
    for (int c = 0; c < 4; c++) out->rk[r][c] = rk[4 * r + c];
  out->nr = (uint32_t)nr;
  return nr;
}

}  // namespace

// aead_aes_ccm_init / aead_aes_eax_init (e_aesccm.cc.inc:275-308,
// e_aeseax.cc:63-95): the key schedule, and EAX's B, P and first-block values
// (computed for CCM keys too; nothing reads them there).
bool cbc_key_setup(const uint8_t *key, size_t key_len, CbcKeyDev *out) {
  uint32_t rk[60];
  const int nr = expand_into(key, key_len, rk, out);
  if (!nr) return false;
  uint32_t l[4] = {0, 0, 0, 0};
  ks_encrypt(rk, nr, l);
  eax_dbl(l, out->eax_b);
  eax_dbl(out->eax_b, out->eax_p);
  for (uint32_t t = 0; t < 3; t++) {
    uint32_t s[4] = {0, 0, 0, t << 24};  // byte 15 = t
    ks_encrypt(rk, nr, s);
    for (int c = 0; c < 4; c++) out->eax_e[t][c] = s[c];
    secure_zero(s, sizeof(s));
  }
  secure_zero(rk, sizeof(rk));
  secure_zero(l, sizeof(l));
  return true;
}

bool mask_key_words(int mask, const uint8_t *key, size_t key_len, uint32_t out[60]) {
  if (mask == kDtlsMaskNone) return true;
  if (mask == kDtlsMaskChaCha) {
    for (int k = 0; k < 32; k++) out[k / 4] |= (uint32_t)key[k] << (8 * (k & 3));
    return true;
  }
  CbcKeyDev ks;
  const bool ok = cbc_key_setup(key, key_len, &ks);
  static_assert(sizeof(ks.rk) == 60 * sizeof(uint32_t), "schedule");
  if (ok) memcpy(out, ks.rk, sizeof(ks.rk));
  secure_zero(&ks, sizeof(ks));
  return ok;
}

namespace {

// FIPS 180-4 6.2.2: one SHA-256 compression of the 64-byte block `blk` into
// the state h.  Plain and slow: it runs twice per key.
void sha256_block(uint32_t h[8], const uint8_t blk[64]) {
  uint32_t w[64];
  auto rotr = [](uint32_t x, int s) { return (x >> s) | (x << (32 - s)); };
  for (int t = 0; t < 16; t++)
    w[t] = (uint32_t)blk[4 * t] << 24 | (uint32_t)blk[4 * t + 1] << 16 |
           (uint32_t)blk[4 * t + 2] << 8 | blk[4 * t + 3];
  for (int t = 16; t < 64; t++) {
    const uint32_t s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
    const uint32_t s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
    w[t] = w[t - 16] + s0 + w[t - 7] + s1;
  }
  uint32_t v[8];
  for (int i = 0; i < 8; i++) v[i] = h[i];
  for (int t = 0; t < 64; t++) {
    const uint32_t a = v[0], e = v[4];
    const uint32_t t1 = v[7] + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) +
                        ((e & v[5]) ^ (~e & v[6])) + kSha256K[t] + w[t];
    const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) +
                        ((a & v[1]) ^ (a & v[2]) ^ (v[1] & v[2]));
    for (int i = 7; i > 0; i--) v[i] = v[i - 1];
    v[4] += t1;
    v[0] = t1 + t2;
  }
  for (int i = 0; i < 8; i++) h[i] += v[i];
  secure_zero(w, sizeof(w));
  secure_zero(v, sizeof(v));
}

// FIPS 180-4 6.1.2: one SHA-1 compression of the 64-byte block `blk` into the
// state h.  Plain and slow, as sha256_block.
void sha1_block(uint32_t h[5], const uint8_t blk[64]) {
  uint32_t w[80];
  auto rotl = [](uint32_t x, int s) { return (x << s) | (x >> (32 - s)); };
  for (int t = 0; t < 16; t++)
    w[t] = (uint32_t)blk[4 * t] << 24 | (uint32_t)blk[4 * t + 1] << 16 |
           (uint32_t)blk[4 * t + 2] << 8 | blk[4 * t + 3];
  for (int t = 16; t < 80; t++) w[t] = rotl(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1);
  uint32_t v[5];
  for (int i = 0; i < 5; i++) v[i] = h[i];
  for (int t = 0; t < 80; t++) {
    const uint32_t b = v[1], c = v[2], d = v[3];
    const uint32_t f = t < 20 ? (b & c) | (~b & d) : t < 40 ? b ^ c ^ d
                       : t < 60 ? (b & c) | (b & d) | (c & d) : b ^ c ^ d;
    const uint32_t k = t < 20 ? 0x5a827999u : t < 40 ? 0x6ed9eba1u
                       : t < 60 ? 0x8f1bbcdcu : 0xca62c1d6u;
    const uint32_t tmp = rotl(v[0], 5) + f + v[4] + k + w[t];
    v[4] = d; v[3] = c; v[2] = rotl(b, 30); v[1] = v[0]; v[0] = tmp;
  }
  for (int i = 0; i < 5; i++) h[i] += v[i];
  secure_zero(w, sizeof(w));
  secure_zero(v, sizeof(v));
}

// InvMixColumns (FIPS-197 5.3.3) of one column, a little-endian word of its
// four bytes: bytes i and i + 2 take 4 (a_i ^ a_{i+2}), then MixColumns.
uint32_t inv_mix_column(uint32_t a) {
  a ^= ks_xtime4(ks_xtime4(a ^ ks_rotr8(a, 2)));
  const uint32_t a1 = ks_rotr8(a, 1);
  return a1 ^ ks_rotr8(a, 2) ^ ks_rotr8(a, 3) ^ ks_xtime4(a ^ a1);
}

// HMAC's two states for a MAC key of mac_len (<= 64) bytes (hmac_init,
// e_aesctrhmac.cc:52-74; HMAC_Init_ex for e_tls.cc): each one compression from
// the hash's initial value (FIPS 180-4 5.3.1, 5.3.3) over the key XOR the pad
// byte, the rest of the block the pad byte itself.  sha1: SHA-1, which uses the
// first five words; else SHA-256.
void hmac_states(const uint8_t *mac_key, size_t mac_len, bool sha1, uint32_t (&inner)[8],
                 uint32_t (&outer)[8]) {
  static const uint32_t kSha1Init[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u,
                                        0xc3d2e1f0u};
  uint8_t blk[64];
  for (int pass = 0; pass < 2; pass++) {
    const uint8_t pad = pass ? 0x5c : 0x36;
    for (size_t i = 0; i < 64; i++) blk[i] = (uint8_t)((i < mac_len ? mac_key[i] : 0) ^ pad);
    uint32_t *h = pass ? outer : inner;
    for (int i = 0; i < (sha1 ? 5 : 8); i++) h[i] = sha1 ? kSha1Init[i] : kSha256Init[i];
    sha1 ? sha1_block(h, blk) : sha256_block(h, blk);
  }
  secure_zero(blk, sizeof(blk));
}

}  // namespace

// aead_aes_ctr_hmac_sha256_init (crypto/cipher/e_aesctrhmac.cc:76-109): the
// key is AES key || 32-byte HMAC key; the schedule and HMAC-SHA256's states.
bool ctr_hmac_key_setup(const uint8_t *key, size_t key_len, AesHmacKeyDev *out) {
  if (key_len != 48 && key_len != 64) return false;
  const size_t aes_len = key_len - 32;
  uint32_t rk[60];
  if (!expand_into(key, aes_len, rk, out)) return false;
  hmac_states(key + aes_len, 32, false, out->inner, out->outer);
  secure_zero(rk, sizeof(rk));
  return true;
}

// aead_tls_init (crypto/cipher/e_tls.cc:61-103): the key is MAC key || AES key;
// HMAC's states over SHA-1 (mac_len 20) or SHA-256 (32).  An opening context
// decrypts: its schedule is the one of the equivalent inverse cipher (FIPS-197
// 5.3.5).
bool tls_cbc_key_setup(const uint8_t *key, size_t key_len, size_t mac_len, bool open,
                       AesHmacKeyDev *out) {
  if ((mac_len != 20 && mac_len != 32) || key_len <= mac_len) return false;
  uint32_t rk[60];
  const int nr = expand_into(key + mac_len, key_len - mac_len, rk, out);
  if (!nr) return false;
  if (open)
    for (int r = 0; r <= nr; r++)
      for (int c = 0; c < 4; c++) {
        const uint32_t w = rk[4 * (nr - r) + c];
        out->rk[r][c] = r > 0 && r < nr ? inv_mix_column(w) : w;
      }
  hmac_states(key, mac_len, mac_len == 20, out->inner, out->outer);
  secure_zero(rk, sizeof(rk));
  return true;
}

namespace {

// Key i's tables from raw key bytes keys[i * key_len ...].  The tables are
// written by their own lane (12,816 B each, scattered 16-byte stores that
// L2 merges into full lines).
__global__ __launch_bounds__(64) void gcm_key_setup_kernel(const uint8_t *__restrict__ keys,
                                                            int key_len, uint64_t n,
                                                            GcmKeyDev *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint8_t k[32];
  for (int j = 0; j < 32; j++) k[j] = j < key_len ? keys[i * key_len + j] : 0;
  gcm_key_tables(k, key_len, out + i);
  ks_wipe(k, sizeof(k));
}

}  // namespace

// n keys of key_len bytes (host memory) -> their tables in device memory
// `out` (n entries), on `s`; returns 0 or a HIP error.  The raw keys pass
// through a device staging buffer that is zeroed before it is freed.
int gcm_key_setup_device(const uint8_t *keys, size_t key_len, size_t n, GcmKeyDev *out,
                         hipStream_t s) {
  if (key_len != 16 && key_len != 24 && key_len != 32) return 1;
  if (!n) return 0;
  uint8_t *raw = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&raw), n * key_len, s);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyAsync(raw, keys, n * key_len, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(gcm_key_setup_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, raw,
                       (int)key_len, (uint64_t)n, out);
    e = hipGetLastError();
  }
  hipMemsetAsync(raw, 0, n * key_len, s);
  hipFreeAsync(raw, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  return (int)(e != hipSuccess ? e : e2);
}

void chacha_key_setup(const uint8_t *key, ChaChaKeyDev *out) {
  for (int i = 0; i < 8; i++) {
    const uint8_t *p = key + 4 * i;
    out->k[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) |
                ((uint32_t)p[3] << 24);
  }
}

}  // namespace bssl_amd
