// ref_ctr_edge_gen.cc -- seals the records of tests/golden/ref_ctr_edge.json
// with the reference library's own EVP_AEADs.  Built and run by
// make_golden_ctr_edge.py against the reference objects in oracle/_ref/; our
// code, linked to theirs.
//
// stdin: one record per line, "aead key nonce ad pt" (hex; "-" for empty).
// stdout: one line per record, "ct tag" (hex; "-" for empty).  The inputs are
// crafted by tests/ctr_edge_util.py so that the counter blocks meet a wrap or
// a carry; this program knows nothing of that.
#include <openssl/aead.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string &s) {
  Bytes out;
  if (s == "-") return out;
  if (s.size() % 2) abort();
  for (size_t i = 0; i < s.size(); i += 2)
    out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

static std::string hex(const uint8_t *p, size_t n) {
  static const char *k = "0123456789abcdef";
  if (!n) return "-";
  std::string s;
  for (size_t i = 0; i < n; i++) {
    s += k[p[i] >> 4];
    s += k[p[i] & 15];
  }
  return s;
}

static const EVP_AEAD *aead_by_name(const std::string &name) {
  if (name == "aes-128-gcm") return EVP_aead_aes_128_gcm();
  if (name == "aes-192-gcm") return EVP_aead_aes_192_gcm();
  if (name == "aes-256-gcm") return EVP_aead_aes_256_gcm();
  if (name == "aes-128-gcm-siv") return EVP_aead_aes_128_gcm_siv();
  if (name == "aes-256-gcm-siv") return EVP_aead_aes_256_gcm_siv();
  if (name == "aes-128-eax") return EVP_aead_aes_128_eax();
  if (name == "aes-256-eax") return EVP_aead_aes_256_eax();
  abort();
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string name, key_h, nonce_h, ad_h, pt_h;
    if (!(in >> name >> key_h >> nonce_h >> ad_h >> pt_h)) abort();
    const Bytes key = unhex(key_h), nonce = unhex(nonce_h), ad = unhex(ad_h), pt = unhex(pt_h);
    EVP_AEAD_CTX ctx;
    if (!EVP_AEAD_CTX_init(&ctx, aead_by_name(name), key.data(), key.size(), 0, nullptr)) abort();
    Bytes ct(pt.size() + 1), tag(EVP_AEAD_MAX_OVERHEAD);
    size_t tag_len = 0;
    if (!EVP_AEAD_CTX_seal_scatter(&ctx, ct.data(), tag.data(), &tag_len, tag.size(), nonce.data(),
                                   nonce.size(), pt.data(), pt.size(), nullptr, 0, ad.data(),
                                   ad.size()))
      abort();
    EVP_AEAD_CTX_cleanup(&ctx);
    printf("%s %s\n", hex(ct.data(), pt.size()).c_str(), hex(tag.data(), tag_len).c_str());
  }
  return 0;
}
