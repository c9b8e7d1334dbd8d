// ref_tls_cbc_records_gen.cc -- seals the records of
// tests/golden/ref_tls_cbc_records.json with the reference library's own
// SSLAEADContext for the TLS 1.1 / 1.2 AES-CBC-HMAC suites (Create with split
// keys, ssl/ssl_aead_ctx.cc:95-114; SealScatter, :299-381), framed as
// do_seal_record frames them (ssl/tls_record.cc:288-299: type, version and the
// fragment's length -- that function is static and needs a whole connection, so
// its header is restated here as in oracle/ref/ref_tls.cc), then opens each
// record with an opening SSLAEADContext (::Open, :226-297) and checks the round
// trip.  Built and run by make_golden_tls_cbc_records.py against the reference
// objects in oracle/_ref/; our code, linked to theirs.
//
// The explicit IV is the reference's RAND_bytes output: different in every
// run, and stored with the record (bytes 5..20 of the prefix).  Keys and
// plaintexts are fill() of oracle/ref/ref_tls.cc with the stored seeds.
#include <openssl/sha.h>
#include <openssl/ssl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "internal.h"  // the reference's ssl/internal.h (SSLAEADContext)

using namespace bssl;

#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      abort();                                                \
    }                                                         \
  } while (0)

namespace {

std::string hex(const uint8_t *p, size_t n) {
  static const char *d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

// Deterministic test bytes: fill() of oracle/ref/ref_tls.cc.
void fill(uint8_t *p, size_t n, uint32_t seed) {
  uint32_t x = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n; i++) {
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    p[i] = (uint8_t)(x >> 7);
  }
}

struct Suite {
  // The cipher suite that selects the AEAD; `alt` where the reference's table
  // no longer lists the first (the record protection is that of the AEAD, the
  // same for every key exchange).
  uint16_t cipher_id, alt;
  const char *aead;
  size_t enc_key_len, mac_len;
};

}  // namespace

int main() {
  const Suite suites[] = {
      {0x002f, 0xc013, "aes-128-cbc-sha1-tls", 16, 20},    // AES128-SHA
      {0x0035, 0xc014, "aes-256-cbc-sha1-tls", 32, 20},    // AES256-SHA
      {0x003c, 0xc027, "aes-128-cbc-sha256-tls", 16, 32},  // AES128-SHA256
  };
  const uint16_t versions[] = {TLS1_1_VERSION, TLS1_2_VERSION};
  const uint64_t seq_starts[] = {0, 0x1234567890ull};
  // The padding edges ((len + mac_len) mod 16 in {15, 0, 1}: 11, 12, 13 + 16 k
  // for SHA-1, 15, 0, 1 + 16 k for SHA-256), the hash-block edges (13 + len =
  // 55, 56, 63, 64 mod 64: 42, 43, 50, 51), and the limit.
  const size_t lens[] = {0, 1, 11, 12, 15, 16, 17, 27, 28, 42, 43, 50, 51, 64, 255, 1350, 16383, 16384};
  const uint8_t types[] = {23, 22, 21};
  printf("[\n");
  bool first_obj = true;
  uint32_t seed = 1000;
  for (const Suite &su : suites) {
    for (uint16_t version : versions) {
      for (uint64_t seq0 : seq_starts) {
        const SSL_CIPHER *cipher = SSL_get_cipher_by_value(su.cipher_id);
        uint16_t used = su.cipher_id;
        if (!cipher) {
          cipher = SSL_get_cipher_by_value(su.alt);
          used = su.alt;
        }
        CHECK(cipher);
        uint8_t enc_key[32], mac_key[32];
        const uint32_t enc_seed = seed++, mac_seed = seed++;
        fill(enc_key, su.enc_key_len, enc_seed);
        fill(mac_key, su.mac_len, mac_seed);
        UniquePtr<SSLAEADContext> sealer = SSLAEADContext::Create(
            evp_aead_seal, version, cipher, Span<const uint8_t>(enc_key, su.enc_key_len),
            Span<const uint8_t>(mac_key, su.mac_len), {});
        UniquePtr<SSLAEADContext> opener = SSLAEADContext::Create(
            evp_aead_open, version, cipher, Span<const uint8_t>(enc_key, su.enc_key_len),
            Span<const uint8_t>(mac_key, su.mac_len), {});
        CHECK(sealer && opener);
        CHECK(sealer->ExplicitNonceLen() == 16);
        printf("%s{\"aead\": \"%s\", \"cipher_id\": %u, \"version\": %u, \"enc_key\": \"%s\", "
               "\"mac_key\": \"%s\", \"seq0\": %llu, \"records\": [\n",
               first_obj ? "" : ",\n", su.aead, used, version, hex(enc_key, su.enc_key_len).c_str(),
               hex(mac_key, su.mac_len).c_str(), (unsigned long long)seq0);
        first_obj = false;
        uint64_t seq = seq0;
        size_t k = 0;
        for (size_t len : lens) {
          const uint8_t type = types[k % 3];
          const uint32_t pt_seed = seed++;
          std::vector<uint8_t> in(len + 1), out(len + 1);
          fill(in.data(), len, pt_seed);
          size_t suffix_len = 0, ct_len = 0;
          CHECK(sealer->SuffixLen(&suffix_len, len, 0) && sealer->CiphertextLen(&ct_len, len, 0));
          CHECK(suffix_len <= 48 && ct_len == 16 + len + suffix_len);
          uint8_t prefix[5 + 16], suffix[48];
          // do_seal_record's header (tls_record.cc:288-299).
          prefix[0] = type;
          prefix[1] = (uint8_t)(version >> 8);
          prefix[2] = (uint8_t)version;
          prefix[3] = (uint8_t)(ct_len >> 8);
          prefix[4] = (uint8_t)ct_len;
          CHECK(sealer->SealScatter(prefix + 5, out.data(), suffix, type, version, seq,
                                    Span<const uint8_t>(prefix, 5), in.data(), len, nullptr, 0));
          // The reference opens what it sealed: the fragment is IV || body || suffix.
          std::vector<uint8_t> frag(prefix + 5, prefix + 21);
          frag.insert(frag.end(), out.begin(), out.begin() + len);
          frag.insert(frag.end(), suffix, suffix + suffix_len);
          CHECK(frag.size() == ct_len);
          Span<uint8_t> plain;
          CHECK(opener->Open(&plain, type, version, seq, Span<const uint8_t>(prefix, 5),
                             Span<uint8_t>(frag.data(), frag.size())));
          CHECK(plain.size() == len && (len == 0 || memcmp(plain.data(), in.data(), len) == 0));
          std::string body;
          if (len <= 64) {
            body = hex(out.data(), len);
          } else {
            uint8_t md[32];
            SHA256(out.data(), len, md);
            body = "sha256:" + hex(md, 32);
          }
          printf("%s {\"seq\": %llu, \"type\": %u, \"len\": %zu, \"pt_seed\": %u, "
                 "\"prefix\": \"%s\", \"body\": \"%s\", \"suffix\": \"%s\"}",
                 k ? ",\n" : "", (unsigned long long)seq, type, len, pt_seed,
                 hex(prefix, 21).c_str(), body.c_str(), hex(suffix, suffix_len).c_str());
          k++;
          seq++;
        }
        printf("]}");
      }
    }
  }
  printf("\n]\n");
  return 0;
}
