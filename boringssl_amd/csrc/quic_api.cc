// quic_api.cc -- the C ABI of BSSL_AMD_QUIC_AEAD (include/bssl_amd/tls.h): one
// direction of one key generation of a QUIC connection over device batches of
// packets (RFC 9001 5).
//
// A call is a chain of launches on the caller's stream and nothing else: the
// prepare step (quic.hip), the bulk kernels of the AEAD over plain records
// whose AD is the header in `out` (launch_desc), and then on seal the tag and
// the header-protection mask, on open the `expected` update.  `expected`, the
// header-protection key and the AEAD key stay on the device; the next packet
// number of a sealing context is the host's, like BSSL_AMD_DTLS_AEAD's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>

#include "bssl_amd/tls.h"
#include "api_internal.h"

using namespace bssl_amd;

struct bssl_amd_quic_aead_st {
  EVP_AEAD_CTX ctx;  // the plain AEAD: the nonces rise by construction (tls.h)
  bool seal;
  int mask;          // DtlsMask
  uint64_t next_pn;  // seal
  uint8_t iv[12];
  QuicState *state;  // device
};

namespace {

constexpr uint32_t kTagLen = 16;

// The scratch of one call, one stream-ordered block freed in stream order on
// every path.  Per packet: the body's offset and length, the header length,
// the packet number (open), the tag, the nonce, the flag and a status byte for
// a caller who passes none.
struct QuicScratch {
  hipStream_t s;
  uint8_t *buf = nullptr;
  uint64_t *body_off, *body_len, *ad_len, *pns;
  uint8_t *tags, *nonce, *valid, *status;
  QuicScratch(hipStream_t stream, uint64_t n) : s(stream) {
    if (bssl_amd::scratch_alloc(reinterpret_cast<void **>(&buf), n * (4 * 8 + 16 + 12 + 2), s) != hipSuccess) {
      buf = nullptr;
      PUT_ERROR(ERR_R_MALLOC_FAILURE);
      return;
    }
    body_off = reinterpret_cast<uint64_t *>(buf);
    body_len = body_off + n;
    ad_len = body_len + n;
    pns = ad_len + n;
    tags = reinterpret_cast<uint8_t *>(pns + n);  // (16-byte aligned: 32 n bytes in)
    nonce = tags + 16 * n;
    valid = nonce + 12 * n;
    status = valid + n;
  }
  ~QuicScratch() {
    if (buf) bssl_amd::scratch_free(buf, s);
  }
  QuicScratch(const QuicScratch &) = delete;
  QuicScratch &operator=(const QuicScratch &) = delete;
};

// The checks both batch calls share; false with the error queued.
bool quic_args_ok(const BSSL_AMD_QUIC_AEAD *q, const BSSL_AMD_QUIC_PACKETS *p, bool want_seal) {
  if (!present(q) || !direction_ok(q->seal, want_seal)) return false;
  if (p && (p->num_packets == 0 ||
            (p->in && p->out &&
             !(want_seal && !p->pn_lengths && (p->pn_length < 1 || p->pn_length > 4)))))
    return true;
  PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
  return false;
}

void fill_prepare(QuicPrepare *k, const BSSL_AMD_QUIC_AEAD *q, const BSSL_AMD_QUIC_PACKETS *p,
                  const QuicScratch &sc) {
  memset(k, 0, sizeof(*k));
  k->n = p->num_packets;
  k->in = p->in;
  k->out = p->out;
  k->offsets = p->offsets;
  k->lengths = p->lengths;
  k->packet_stride = p->packet_stride;
  k->packet_len = p->packet_len;
  k->pn_offsets = p->pn_offsets;
  k->pn_offset = p->pn_offset;
  memcpy(k->iv, q->iv, 12);
  k->open = !q->seal;
  k->nonces = sc.nonce;
  k->valid = sc.valid;
  k->tags = sc.tags;
  k->body_offsets = sc.body_off;
  k->body_lengths = sc.body_len;
  k->ad_lengths = sc.ad_len;
  k->pns = sc.pns;
  k->packet_numbers = p->packet_numbers;
  k->state = q->state;
}

// The packets as the bulk kernels see them: record i is the body, its AD the
// header that the prepare step left in `out`, its tag in the scratch.
BatchDesc batch_desc(const BSSL_AMD_QUIC_PACKETS *p, const QuicScratch &sc) {
  BatchDesc d;
  memset(&d, 0, sizeof(d));
  d.in = p->in;
  d.out = p->out;
  d.offsets = sc.body_off;
  d.lengths = sc.body_len;
  d.nonces = sc.nonce;
  d.nonce_len = 12;
  d.ad = p->out;
  d.ad_offsets = p->offsets;
  d.ad_stride = p->packet_stride;
  d.ad_lengths = sc.ad_len;
  d.tags = sc.tags;
  d.tag_stride = kTagLen;
  d.tag_len = kTagLen;
  // The steps after the bulk kernels read the status: always an array.
  d.status = p->status ? p->status : sc.status;
  d.num_records = p->num_packets;
  d.num_keys = 1;
  d.valid = sc.valid;
  d.any_align = 1;  // a body starts where its header ends
  return d;
}

int quic_seal(BSSL_AMD_QUIC_AEAD *q, const BSSL_AMD_QUIC_PACKETS *p, void *stream) {
  const uint64_t n = p->num_packets;
  if (n == 0) return 1;
  if (q->next_pn > kQuicMaxPacketNumber || n - 1 > kQuicMaxPacketNumber - q->next_pn) {
    PUT_ERROR(ERR_R_OVERFLOW);
    return 0;
  }
  const KeyMaterial *km = state_of(&q->ctx)->km;
  if (!on_key_device(km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  QuicScratch sc(s, n);
  if (!sc.buf) return 0;
  BatchDesc d = batch_desc(p, sc);
#ifndef BSSL_AMD_QUIC_NO_UNIFORM_SEAL  // (the A/B of DESIGN.md 4.7e: tools/ab_build.sh)
  // One shape for every packet, and one that seals: the bodies are a uniform
  // batch from base pointers shifted past the header, which keeps the
  // ChaCha20-Poly1305 kernel's uniform path (no per-record loads, no length
  // order) instead of the ragged one.  AES-GCM does not take it: its uniform
  // kernels were 1.39x slower on unaligned bodies than its ragged ones
  // (DESIGN.md 4.7e).
  const uint64_t hdr = (uint64_t)p->pn_offset + p->pn_length;
  if (km->aead->kind == kAeadChaChaPoly && !p->lengths && !p->pn_offsets && !p->pn_lengths &&
      p->pn_offset != 0 &&
      hdr <= p->packet_len && p->packet_len - p->pn_offset >= 4) {
    d.in = p->in + hdr;
    d.out = p->out + hdr;
    d.offsets = p->offsets;
    d.record_stride = p->packet_stride;
    d.lengths = nullptr;
    d.record_len = p->packet_len - hdr;
    d.ad_lengths = nullptr;
    d.ad_len = hdr;
    d.valid = nullptr;
  }
#endif
  QuicPrepare k;
  fill_prepare(&k, q, p, sc);
  k.pn_lengths = p->pn_lengths;
  k.pn_length = p->pn_length;
  k.next_pn = q->next_pn;
  Timed prepare(s);
  bool ok = launch_quic_prepare(k, q->mask, stream) == 0;
  prepare.stop();
  secure_zero(&k, sizeof(k));
  ok = ok && launch_desc(km, d, false, stream) == 0;
  if (ok) {
    Timed protect(s);
    const QuicProtect m = {n,           p->out,      p->offsets, p->lengths, p->packet_stride,
                           p->packet_len, sc.body_off, sc.body_len, sc.tags,   d.status,
                           p->out_lengths, q->state};
    ok = launch_quic_protect(m, q->mask, stream) == 0;
    protect.stop();
  }
  if (ok) q->next_pn += n;
  return finish(ok);
}

int quic_open(BSSL_AMD_QUIC_AEAD *q, const BSSL_AMD_QUIC_PACKETS *p, void *stream) {
  const uint64_t n = p->num_packets;
  if (n == 0) return 1;
  const KeyMaterial *km = state_of(&q->ctx)->km;
  if (!on_key_device(km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  QuicScratch sc(s, n);
  if (!sc.buf) return 0;
  const BatchDesc d = batch_desc(p, sc);
  QuicPrepare k;
  fill_prepare(&k, q, p, sc);
  k.header_lengths = p->header_lengths;
  Timed prepare(s);
  bool ok = launch_quic_prepare(k, q->mask, stream) == 0;
  prepare.stop();
  secure_zero(&k, sizeof(k));
  ok = ok && launch_desc(km, d, true, stream) == 0;
  if (ok) {
    Timed expected(s);
    const QuicExpected e = {n, d.status, sc.pns, sc.body_len, p->out_lengths, q->state};
    ok = launch_quic_expected(e, stream) == 0;
    expected.stop();
  }
  return finish(ok);
}

// get_expected / set_expected: an opening context on its device.
bool expected_ok(const BSSL_AMD_QUIC_AEAD *q) {
  if (!present(q)) return false;
  if (q->seal) {
    PUT_ERROR(CIPHER_R_INVALID_OPERATION);
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

BSSL_AMD_QUIC_AEAD *BSSL_AMD_QUIC_AEAD_new(enum evp_aead_direction_t direction,
                                           const EVP_AEAD *aead, const uint8_t *key,
                                           size_t key_len, const uint8_t *iv, size_t iv_len,
                                           const uint8_t *hp_key, size_t hp_key_len,
                                           uint64_t next_pn) {
  // All checks before any GPU call, in BSSL_AMD_DTLS_AEAD_new's order.
  if (!aead || !key || !iv || !hp_key || next_pn > kQuicMaxPacketNumber) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return nullptr;
  }
  if (aead->kind == kAeadAesCtrHmac || aead->kind == kAeadTlsCbc) {
    PUT_ERROR(CIPHER_R_CTRL_NOT_IMPLEMENTED);
    return nullptr;
  }
  const bool chacha = aead == EVP_aead_chacha20_poly1305();
  if ((!chacha && aead != EVP_aead_aes_128_gcm() && aead != EVP_aead_aes_256_gcm()) ||
      key_len != aead->key_len || iv_len != 12 || hp_key_len != aead->key_len) {
    PUT_ERROR(CIPHER_R_UNSUPPORTED_KEY_SIZE);
    return nullptr;
  }
  BSSL_AMD_QUIC_AEAD *q = new (std::nothrow) bssl_amd_quic_aead_st;
  if (!q) {
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  EVP_AEAD_CTX_zero(&q->ctx);
  if (!EVP_AEAD_CTX_init_with_direction(&q->ctx, aead, key, key_len, EVP_AEAD_DEFAULT_TAG_LENGTH,
                                        direction)) {
    delete q;
    return nullptr;
  }
  q->seal = direction == evp_aead_seal;
  q->mask = chacha ? kDtlsMaskChaCha : aead->key_len == 16 ? kDtlsMaskAes128 : kDtlsMaskAes256;
  q->next_pn = next_pn;
  memcpy(q->iv, iv, 12);
  q->state = nullptr;
  // The device state: expected 0 and the header-protection key, expanded once.
  QuicState host;
  memset(&host, 0, sizeof(host));
  bool ok = mask_key_words(q->mask, hp_key, hp_key_len, host.hp);
  ok = ok && hipMalloc(reinterpret_cast<void **>(&q->state), sizeof(QuicState)) == hipSuccess;
  if (!ok) q->state = nullptr;
  ok = ok && hipMemcpy(q->state, &host, sizeof(host), hipMemcpyHostToDevice) == hipSuccess;
  secure_zero(&host, sizeof(host));
  if (!ok) {
    BSSL_AMD_QUIC_AEAD_free(q);
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  return q;
}

void BSSL_AMD_QUIC_AEAD_free(BSSL_AMD_QUIC_AEAD *q) {
  if (!q) return;
  if (q->state) {
    DeviceGuard g(state_of(&q->ctx)->km->device);
    // As free_keys: drain the device, wipe, drain, free.
    hipDeviceSynchronize();
    hipMemset(q->state, 0, sizeof(QuicState));
    hipDeviceSynchronize();
    hipFree(q->state);
  }
  EVP_AEAD_CTX_cleanup(&q->ctx);
  secure_zero(q->iv, sizeof(q->iv));
  delete q;
}

uint64_t BSSL_AMD_QUIC_AEAD_next_packet_number(const BSSL_AMD_QUIC_AEAD *q) { return q->next_pn; }

int BSSL_AMD_QUIC_AEAD_get_expected(BSSL_AMD_QUIC_AEAD *q, uint64_t *expected, void *hip_stream) {
  if (!expected_ok(q) || !present(expected)) return 0;
  if (!on_key_device(state_of(&q->ctx)->km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  uint64_t e = 0;
  if (hipMemcpyAsync(&e, &q->state->expected, sizeof(e), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return finish(false);
  *expected = e;
  return 1;
}

int BSSL_AMD_QUIC_AEAD_set_expected(BSSL_AMD_QUIC_AEAD *q, uint64_t expected, void *hip_stream) {
  if (!expected_ok(q)) return 0;
  if (expected > kQuicMaxPacketNumber + 1) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  if (!on_key_device(state_of(&q->ctx)->km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  // (The copy reads this frame: wait until it has.)
  return finish(hipMemcpyAsync(&q->state->expected, &expected, sizeof(expected),
                               hipMemcpyHostToDevice, s) == hipSuccess &&
                hipStreamSynchronize(s) == hipSuccess);
}

int BSSL_AMD_QUIC_AEAD_seal_packets_device(BSSL_AMD_QUIC_AEAD *q, const BSSL_AMD_QUIC_PACKETS *p,
                                           void *hip_stream) {
  return quic_args_ok(q, p, true) ? quic_seal(q, p, hip_stream) : 0;
}

int BSSL_AMD_QUIC_AEAD_open_packets_device(BSSL_AMD_QUIC_AEAD *q, const BSSL_AMD_QUIC_PACKETS *p,
                                           void *hip_stream) {
  return quic_args_ok(q, p, false) ? quic_open(q, p, hip_stream) : 0;
}

}  // extern "C"
