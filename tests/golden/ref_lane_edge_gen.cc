// ref_lane_edge_gen.cc -- runs the records of tests/golden/ref_lane_edge.json.xz
// through the reference library's own EVP_AEADs.  Built and run by
// make_golden_lane_edge.py against the reference objects in oracle/_ref/; our
// code, linked to theirs.
//
// stdin: one record per line, "aead direction key nonce ad in" (hex; "-" for
// empty; direction "seal" or "open"; the AES-CTR-HMAC names carry their tag
// length as "name:N").  stdout: one line per record, "ret out_len sha256": the
// call's return value, the output length it reported and the SHA-256 of those
// output bytes.  The inputs are made by tests/lane_edge_util.py; this program
// knows nothing of them.
#include <openssl/aead.h>
#include <openssl/sha.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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

static const EVP_AEAD *aead_by_name(const std::string &name) {
  if (name == "aes-128-ccm-bluetooth") return EVP_aead_aes_128_ccm_bluetooth();
  if (name == "aes-128-ccm-bluetooth-8") return EVP_aead_aes_128_ccm_bluetooth_8();
  if (name == "aes-128-ccm-matter") return EVP_aead_aes_128_ccm_matter();
  if (name == "aes-128-eax") return EVP_aead_aes_128_eax();
  if (name == "aes-256-eax") return EVP_aead_aes_256_eax();
  if (name == "aes-128-ctr-hmac-sha256") return EVP_aead_aes_128_ctr_hmac_sha256();
  if (name == "aes-256-ctr-hmac-sha256") return EVP_aead_aes_256_ctr_hmac_sha256();
  if (name == "aes-128-cbc-sha1-tls") return EVP_aead_aes_128_cbc_sha1_tls();
  if (name == "aes-256-cbc-sha1-tls") return EVP_aead_aes_256_cbc_sha1_tls();
  if (name == "aes-128-cbc-sha256-tls") return EVP_aead_aes_128_cbc_sha256_tls();
  fprintf(stderr, "unknown AEAD %s\n", name.c_str());
  abort();
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string name, dir, key_h, nonce_h, ad_h, in_h;
    if (!(in >> name >> dir >> key_h >> nonce_h >> ad_h >> in_h)) abort();
    size_t tag_len = EVP_AEAD_DEFAULT_TAG_LENGTH;
    const size_t colon = name.find(':');
    if (colon != std::string::npos) {
      tag_len = strtoul(name.c_str() + colon + 1, nullptr, 10);
      name.resize(colon);
    }
    if (dir != "seal" && dir != "open") abort();
    const Bytes key = unhex(key_h), nonce = unhex(nonce_h), ad = unhex(ad_h), data = unhex(in_h);
    const EVP_AEAD *aead = aead_by_name(name);
    EVP_AEAD_CTX ctx;
    EVP_AEAD_CTX_zero(&ctx);
    if (!EVP_AEAD_CTX_init_with_direction(&ctx, aead, key.data(), key.size(), tag_len,
                                          dir == "seal" ? evp_aead_seal : evp_aead_open))
      abort();
    Bytes out(data.size() + EVP_AEAD_max_overhead(aead) + 1);
    size_t out_len = 0;
    const int ret =
        dir == "seal" ? EVP_AEAD_CTX_seal(&ctx, out.data(), &out_len, out.size(), nonce.data(),
                                          nonce.size(), data.data(), data.size(), ad.data(), ad.size())
                      : EVP_AEAD_CTX_open(&ctx, out.data(), &out_len, out.size(), nonce.data(),
                                          nonce.size(), data.data(), data.size(), ad.data(), ad.size());
    EVP_AEAD_CTX_cleanup(&ctx);
    uint8_t d[32];
    SHA256(out.data(), out_len, d);
    printf("%d %zu ", ret, out_len);
    for (int i = 0; i < 32; i++) printf("%02x", d[i]);
    printf("\n");
  }
  return 0;
}
