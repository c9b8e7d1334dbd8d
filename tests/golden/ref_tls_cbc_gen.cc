// ref_tls_cbc_gen.cc -- seals the records of tests/golden/ref_tls_cbc.json with
// the reference library's own TLS AES-CBC-HMAC AEADs (EVP_AEAD_CTX_seal through
// EVP_AEAD_CTX_init_with_direction), opens each again, and prints them as JSON.
// Built and run by make_golden_tls_cbc.py against the reference objects in
// oracle/_ref/; our code, linked to theirs.
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

#include <set>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      abort();                                                \
    }                                                         \
  } while (0)

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
  size_t key_len, mac_len;
};
static const Aead kAeads[] = {
    {"aes-128-cbc-sha1-tls", EVP_aead_aes_128_cbc_sha1_tls, 36, 20},
    {"aes-256-cbc-sha1-tls", EVP_aead_aes_256_cbc_sha1_tls, 52, 20},
    {"aes-128-cbc-sha256-tls", EVP_aead_aes_128_cbc_sha256_tls, 48, 32},
};

static bool g_first = true;

static void record(const Aead &a, size_t pt_len) {
  const std::string label = std::string(a.name) + "/msg" + std::to_string(pt_len);
  const Bytes key = gen(label + "/key", a.key_len), nonce = gen(label + "/nonce", 16),
              ad = gen(label + "/ad", 11), pt = gen(label + "/pt", pt_len);
  EVP_AEAD_CTX ctx;
  EVP_AEAD_CTX_zero(&ctx);  // (these AEADs' init leaves ctx.tag_len as it finds it)
  CHECK(EVP_AEAD_CTX_init_with_direction(&ctx, a.get(), key.data(), key.size(), 0, evp_aead_seal));
  Bytes wire(pt_len + EVP_AEAD_max_overhead(a.get()));
  size_t got = 0, want_tag = 0;
  CHECK(EVP_AEAD_CTX_tag_len(&ctx, &want_tag, pt_len, 0));
  CHECK(EVP_AEAD_CTX_seal(&ctx, wire.data(), &got, wire.size(), nonce.data(), nonce.size(),
                         pt.data(), pt.size(), ad.data(), ad.size()));
  EVP_AEAD_CTX_cleanup(&ctx);
  CHECK(got == pt_len + want_tag);
  wire.resize(got);
  // The reference opens what it sealed, to the same plaintext.
  EVP_AEAD_CTX_zero(&ctx);
  CHECK(EVP_AEAD_CTX_init_with_direction(&ctx, a.get(), key.data(), key.size(), 0, evp_aead_open));
  Bytes back(got);
  size_t back_len = 0;
  CHECK(EVP_AEAD_CTX_open(&ctx, back.data(), &back_len, back.size(), nonce.data(), nonce.size(),
                         wire.data(), wire.size(), ad.data(), ad.size()));
  EVP_AEAD_CTX_cleanup(&ctx);
  CHECK(back_len == pt_len && std::equal(pt.begin(), pt.end(), back.begin()));
  printf("%s{\"aead\": \"%s\", \"label\": \"%s\", \"pt_len\": %zu, \"tag_len\": %zu",
         g_first ? "" : ",\n", a.name, label.c_str(), pt_len, want_tag);
  g_first = false;
  if (pt_len <= 64) {
    printf(", \"wire\": \"%s\"", hex(wire.data(), got).c_str());
  } else {
    uint8_t d[32];
    SHA256(wire.data(), wire.size(), d);
    printf(", \"sha256\": \"%s\"", hex(d, 32).c_str());
  }
  printf("}");
}

int main() {
  // Every length 0..130: every residue of (len + mac_len) mod 16 several times
  // over, the first hash block full at 51 (13 + 51 = 64), SHA's padding
  // spilling into a second block from 43 on (13 + 43 = 56).  Then a TLS record
  // of 1350 and of 16384 bytes, and the 16-bit length wrap.
  std::set<size_t> lens = {1350, 16384, 65535, 65536, 65541};
  for (size_t i = 0; i <= 130; i++) lens.insert(i);
  printf("[\n");
  for (const Aead &a : kAeads)
    for (size_t m : lens) record(a, m);
  printf("\n]\n");
  return 0;
}
