// ref_ccm_eax_gen.cc -- seals the records of tests/golden/ref_ccm_eax.json with
// the reference library's own AES-CCM and AES-EAX (EVP_AEAD_CTX_seal_scatter)
// and prints them as JSON.  Built and run by make_golden_ccm_eax.py against
// the reference objects in oracle/_ref/; our code, linked to theirs.
//
// Inputs follow one rule, restated in tests/test_ccm_eax_ref.py: the n bytes
// named `label` are the first n bytes of SHA-256(label || be32(0)) ||
// SHA-256(label || be32(1)) || ...; a record labelled R uses R/key, R/nonce,
// R/ad and R/pt.  Only the two counter-carry records carry a searched nonce
// (stored in the fixture like every nonce).
#include <openssl/aead.h>
#include <openssl/aes.h>
#include <openssl/sha.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;

static Bytes gen(const std::string &label, size_t n) {
  Bytes out;
  for (uint32_t i = 0; out.size() < n; i++) {
    Bytes in(label.begin(), label.end());
    for (int s = 24; s >= 0; s -= 8) in.push_back((uint8_t)(i >> s));
    uint8_t d[32];
    SHA256(in.data(), in.size(), d);
    out.insert(out.end(), d, d + 32);
  }
  out.resize(n);
  return out;
}

static std::string hex(const uint8_t *p, size_t n) {
  static const char *k = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) {
    s += k[p[i] >> 4];
    s += k[p[i] & 15];
  }
  return s;
}

struct Aead {
  const char *name;
  const EVP_AEAD *(*get)(void);
  size_t key_len, tag_len;
  bool eax;
};
static const Aead kAeads[] = {
    {"aes-128-ccm-bluetooth", EVP_aead_aes_128_ccm_bluetooth, 16, 4, false},
    {"aes-128-ccm-bluetooth-8", EVP_aead_aes_128_ccm_bluetooth_8, 16, 8, false},
    {"aes-128-ccm-matter", EVP_aead_aes_128_ccm_matter, 16, 16, false},
    {"aes-128-eax", EVP_aead_aes_128_eax, 16, 16, true},
    {"aes-256-eax", EVP_aead_aes_256_eax, 32, 16, true},
};

static bool g_first = true;

static void record(const Aead &a, const std::string &label, const Bytes &nonce, size_t pt_len,
                   size_t ad_len) {
  const Bytes key = gen(label + "/key", a.key_len), ad = gen(label + "/ad", ad_len),
              pt = gen(label + "/pt", pt_len);
  EVP_AEAD_CTX ctx;
  if (!EVP_AEAD_CTX_init(&ctx, a.get(), key.data(), key.size(), 0, nullptr)) abort();
  Bytes ct(pt_len + 1), tag(EVP_AEAD_MAX_OVERHEAD);
  size_t tag_len = 0;
  const int ok = EVP_AEAD_CTX_seal_scatter(&ctx, ct.data(), tag.data(), &tag_len, tag.size(),
                                           nonce.data(), nonce.size(), pt.data(), pt.size(),
                                           nullptr, 0, ad.data(), ad.size());
  EVP_AEAD_CTX_cleanup(&ctx);
  printf("%s{\"aead\": \"%s\", \"label\": \"%s\", \"nonce\": \"%s\", \"pt_len\": %zu, "
         "\"ad_len\": %zu, \"ok\": %s",
         g_first ? "" : ",\n", a.name, label.c_str(), hex(nonce.data(), nonce.size()).c_str(),
         pt_len, ad_len, ok ? "true" : "false");
  g_first = false;
  if (ok) {
    if (tag_len != a.tag_len) abort();
    if (pt_len <= 64) {
      printf(", \"ct\": \"%s\", \"tag\": \"%s\"", hex(ct.data(), pt_len).c_str(),
             hex(tag.data(), tag_len).c_str());
    } else {
      Bytes all(ct.begin(), ct.begin() + pt_len);
      all.insert(all.end(), tag.begin(), tag.begin() + tag_len);
      uint8_t d[32];
      SHA256(all.data(), all.size(), d);
      printf(", \"sha256\": \"%s\"", hex(d, 32).c_str());
    }
  }
  printf("}");
}

// EAX's N = OMAC^0(nonce) for a 16-byte nonce, by the reference's AES alone:
// E_K(E_K(0^128) ^ nonce ^ B), B = 2 E_K(0^128) in GF(2^128) (big-endian,
// reduced by 0x87).  Searches the nonce's last 8 bytes for low32(N) >=
// 0xfffffff0, so that a 512-byte message carries out of the counter's low word.
static Bytes carry_nonce(const Bytes &key, const Bytes &prefix8) {
  AES_KEY ks;
  if (AES_set_encrypt_key(key.data(), (unsigned)key.size() * 8, &ks) != 0) abort();
  uint8_t l[16] = {0}, b[16], e0[16];
  AES_encrypt(l, l, &ks);
  for (int i = 0; i < 16; i++) b[i] = (uint8_t)((l[i] << 1) | (i < 15 ? l[i + 1] >> 7 : 0));
  if (l[0] & 0x80) b[15] ^= 0x87;
  memset(e0, 0, 16);
  AES_encrypt(e0, e0, &ks);  // E_K(0^15 || 0)
  uint8_t base[16];
  for (int i = 0; i < 16; i++) base[i] = e0[i] ^ b[i];
  Bytes nonce(16);
  memcpy(nonce.data(), prefix8.data(), 8);
  for (uint64_t c = 0;; c++) {
    for (int i = 0; i < 8; i++) nonce[8 + i] = (uint8_t)(c >> (56 - 8 * i));
    uint8_t x[16];
    for (int i = 0; i < 16; i++) x[i] = base[i] ^ nonce[i];
    AES_encrypt(x, x, &ks);
    if (x[12] == 0xff && x[13] == 0xff && x[14] == 0xff && x[15] >= 0xf0) return nonce;
  }
}

int main() {
  static const size_t kMsg[] = {0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1350, 4097, 65535};
  static const size_t kAd[] = {0, 1, 13, 14, 15, 16, 30, 65279, 65280};
  printf("[\n");
  for (const Aead &a : kAeads) {
    for (size_t nonce_len : {(size_t)16, (size_t)12}) {
      if (!a.eax) {
        if (nonce_len != 16) continue;
        nonce_len = 13;
      }
      const std::string base = std::string(a.name) + "/n" + std::to_string(nonce_len);
      auto one = [&](const std::string &what, size_t pt_len, size_t ad_len) {
        const std::string label = base + "/" + what;
        record(a, label, gen(label + "/nonce", nonce_len), pt_len, ad_len);
      };
      for (size_t m : kMsg) one("msg" + std::to_string(m), m, 13);
      // CCM (L = 2): over the limit, the reference returns 0; EAX has none.
      one("msg65536", 65536, 13);
      if (a.eax) one("msg70001", 70001, 13);
      for (size_t d : kAd) one("ad" + std::to_string(d), 33, d);
      if (a.eax && nonce_len == 16) {
        const std::string label = base + "/carry";
        const Bytes key = gen(label + "/key", a.key_len);
        record(a, label, carry_nonce(key, gen(label + "/nonce", 8)), 512, 13);
      }
    }
  }
  printf("\n]\n");
  return 0;
}
