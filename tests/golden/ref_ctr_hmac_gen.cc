// ref_ctr_hmac_gen.cc -- seals the records of tests/golden/ref_ctr_hmac.json
// with the reference library's own AES-128/256-CTR-HMAC-SHA256
// (EVP_AEAD_CTX_seal_scatter) and prints them as JSON.  Built and run by
// make_golden_ctr_hmac.py against the reference objects in oracle/_ref/; our
// code, linked to theirs.
//
// Inputs follow the rule of ref_ccm_eax_gen.cc, restated in
// tests/ccm_eax_ref.py (derive): the n bytes named `label` are the first n
// bytes of SHA-256(label || be32(0)) || SHA-256(label || be32(1)) || ...; a
// record labelled R uses R/key, R/nonce, R/ad and R/pt, so the fixture stores
// outputs only.
#include <openssl/aead.h>
#include <openssl/sha.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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
  size_t key_len;
};
static const Aead kAeads[] = {
    {"aes-128-ctr-hmac-sha256", EVP_aead_aes_128_ctr_hmac_sha256, 48},
    {"aes-256-ctr-hmac-sha256", EVP_aead_aes_256_ctr_hmac_sha256, 64},
};

static bool g_first = true;

// tag_len 0: the default (32).
static void record(const Aead &a, const std::string &label, size_t pt_len, size_t ad_len,
                   size_t tag_len) {
  const Bytes key = gen(label + "/key", a.key_len), nonce = gen(label + "/nonce", 12),
              ad = gen(label + "/ad", ad_len), pt = gen(label + "/pt", pt_len);
  EVP_AEAD_CTX ctx;
  if (!EVP_AEAD_CTX_init(&ctx, a.get(), key.data(), key.size(), tag_len, nullptr)) abort();
  Bytes ct(pt_len + 1), tag(EVP_AEAD_MAX_OVERHEAD);
  size_t got = 0;
  if (!EVP_AEAD_CTX_seal_scatter(&ctx, ct.data(), tag.data(), &got, tag.size(), nonce.data(),
                                 nonce.size(), pt.data(), pt.size(), nullptr, 0, ad.data(),
                                 ad.size()))
    abort();
  EVP_AEAD_CTX_cleanup(&ctx);
  if (got != (tag_len ? tag_len : 32)) abort();
  printf("%s{\"aead\": \"%s\", \"label\": \"%s\", \"pt_len\": %zu, \"ad_len\": %zu, "
         "\"tag_len\": %zu",
         g_first ? "" : ",\n", a.name, label.c_str(), pt_len, ad_len, got);
  g_first = false;
  if (pt_len <= 64) {
    printf(", \"ct\": \"%s\", \"tag\": \"%s\"", hex(ct.data(), pt_len).c_str(),
           hex(tag.data(), got).c_str());
  } else {
    Bytes all(ct.begin(), ct.begin() + pt_len);
    all.insert(all.end(), tag.begin(), tag.begin() + got);
    uint8_t d[32];
    SHA256(all.data(), all.size(), d);
    printf(", \"sha256\": \"%s\"", hex(d, 32).c_str());
  }
  printf("}");
}

int main() {
  // Both sides of every 16- and 64-byte edge, of SHA's padding edge (55, 56;
  // 119, 120) and of the page; with the 28-byte header, AD 36 fills the first
  // hash block and AD 100 the second.
  static const size_t kMsg[] = {0,   1,   15,  16,  17,  31,  32,  33,   47,   48,  49,
                                55,  56,  57,  63,  64,  65,  111, 119,  120,  121, 127,
                                128, 129, 255, 256, 257, 1350, 4095, 4096, 4097};
  static const size_t kAd[] = {0, 1, 35, 36, 37, 63, 64, 65, 99, 100, 101, 4097};
  static const size_t kTag[] = {1, 16, 31};
  printf("[\n");
  for (const Aead &a : kAeads) {
    const std::string base = a.name;
    for (size_t m : kMsg)
      for (size_t d : {(size_t)0, (size_t)13})
        record(a, base + "/msg" + std::to_string(m) + "/ad" + std::to_string(d), m, d, 0);
    for (size_t d : kAd)
      for (size_t m : {(size_t)0, (size_t)57})
        record(a, base + "/ad" + std::to_string(d) + "/msg" + std::to_string(m), m, d, 0);
    for (size_t t : kTag)
      for (size_t m : {(size_t)57, (size_t)1350})
        record(a, base + "/tag" + std::to_string(t) + "/msg" + std::to_string(m), m, 13, t);
  }
  printf("\n]\n");
  return 0;
}
