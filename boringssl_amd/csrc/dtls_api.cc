// dtls_api.cc -- the C ABI of BSSL_AMD_DTLS_AEAD (include/bssl_amd/tls.h): one
// direction of one epoch of a DTLS 1.2 / 1.3 association over device batches.
//
// dtls_seal_record / dtls_open_record (ssl/dtls_record.cc:481-584, 292-425)
// for a batch of records.  A call is a chain of launches on the caller's
// stream and nothing else: the prepare step (dtls.hip), the bulk kernels of
// the AEAD over plain records (launch_desc), and then on seal the DTLS 1.3
// record-number mask, on open the DTLS 1.3 strip (tls_pad.hip) and the replay
// window.  The window, the record-number key and the AEAD key stay on the
// device; the write sequence number is the host's, like BSSL_AMD_TLS_AEAD's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>

#include "bssl_amd/tls.h"
#include "api_internal.h"

using namespace bssl_amd;

struct bssl_amd_dtls_aead_st {
  EVP_AEAD_CTX ctx;  // the plain AEAD: the nonces rise by construction (tls.h)
  bool seal;
  bool dtls13;
  bool xor_nonce;    // fixed IV XOR the sequence number vs 4-byte IV || explicit nonce
  int mask;          // DtlsMask
  uint16_t epoch;
  uint64_t seq;      // seal: the next sequence number
  uint8_t fixed_iv[12];
  DtlsState *state;  // device
  uint32_t prefix_len() const { return dtls13 ? 5 : xor_nonce ? 13 : 21; }
  uint32_t ad_stride() const { return dtls13 ? 5 : 13; }
};

namespace {

constexpr uint32_t kTagLen = 16;

// The scratch of one call, one stream-ordered block freed in stream order on
// every path.  Per record: the fragment length (DTLS 1.3 seal), the sequence
// number and the AD length (open), the nonce, the AD, the flag, a status byte
// and a type byte for a caller who passes none; for an open the window's hash
// table, workgroup maxima and old state (DtlsWindow).
struct DtlsScratch {
  hipStream_t s;
  uint8_t *buf = nullptr;
  uint64_t *frag_len, *seqs, *ad_len, *table, *block_max, *old;
  uint64_t table_slots = 0;
  uint8_t *nonce, *ad, *valid, *status, *types;
  DtlsScratch(hipStream_t stream, uint64_t n, uint32_t ad_stride, bool open) : s(stream) {
    const uint64_t nb = (n + 255) / 256;
    if (open)
      for (table_slots = 512; table_slots < 2 * n;) table_slots *= 2;
    const uint64_t words = 3 * n + 2 * table_slots + nb + 5;
    if (bssl_amd::scratch_alloc(reinterpret_cast<void **>(&buf), 8 * words + n * (12 + ad_stride + 3), s) !=
        hipSuccess) {
      buf = nullptr;
      PUT_ERROR(ERR_R_MALLOC_FAILURE);
      return;
    }
    frag_len = reinterpret_cast<uint64_t *>(buf);
    seqs = frag_len + n;
    ad_len = seqs + n;
    table = ad_len + n;
    block_max = table + 2 * table_slots;
    old = block_max + nb;
    nonce = reinterpret_cast<uint8_t *>(old + 5);
    ad = nonce + 12 * n;
    valid = ad + ad_stride * n;
    status = valid + n;
    types = status + n;
  }
  ~DtlsScratch() {
    if (buf) bssl_amd::scratch_free(buf, s);
  }
  DtlsScratch(const DtlsScratch &) = delete;
  DtlsScratch &operator=(const DtlsScratch &) = delete;
};

// The checks both record calls share; false with the error queued.
bool dtls_args_ok(const BSSL_AMD_DTLS_AEAD *t, const BSSL_AMD_DTLS_RECORDS *r, bool want_seal) {
  if (!present(t) || !direction_ok(t->seal, want_seal)) return false;
  if (r && (r->num_records == 0 ||
            (r->in && r->out && r->prefix && r->suffix &&
             !(!want_seal && t->dtls13 && !r->out_lengths))))
    return true;
  PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
  return false;
}

void fill_prepare(DtlsPrepare *p, const BSSL_AMD_DTLS_AEAD *t, const BSSL_AMD_DTLS_RECORDS *r,
                  const DtlsScratch &sc) {
  memset(p, 0, sizeof(*p));
  p->n = r->num_records;
  p->offsets = r->offsets;
  p->lengths = r->lengths;
  p->record_stride = r->record_stride;
  p->record_len = r->record_len;
  memcpy(p->fixed_iv, t->fixed_iv, 12);
  p->epoch = t->epoch;
  p->open = !t->seal;
  p->dtls13 = t->dtls13;
  p->xor_nonce = t->xor_nonce;
  p->prefix_len = t->prefix_len();
  p->ad_stride = t->ad_stride();
  p->prefix = r->prefix;
  p->suffix = r->suffix;
  p->nonces = sc.nonce;
  p->ad = sc.ad;
  p->valid = sc.valid;
  p->record_numbers = r->record_numbers;
  p->state = t->state;
}

BatchDesc batch_desc(const BSSL_AMD_DTLS_AEAD *t, const BSSL_AMD_DTLS_RECORDS *r,
                     const DtlsScratch &sc) {
  BatchDesc d;
  memset(&d, 0, sizeof(d));
  d.in = r->in;
  d.out = r->out;
  d.offsets = r->offsets;
  d.lengths = r->lengths;
  d.record_stride = r->record_stride;
  d.record_len = r->record_len;
  d.nonces = sc.nonce;
  d.nonce_len = 12;
  d.ad = sc.ad;
  d.ad_stride = t->ad_stride();
  d.ad_len = t->ad_stride();
  d.tags = r->suffix;
  d.tag_stride = kTagLen;
  d.tag_len = kTagLen;
  // The steps after the bulk kernels read the status: always an array.
  d.status = r->status ? r->status : sc.status;
  d.num_records = r->num_records;
  d.num_keys = 1;
  d.valid = sc.valid;
  return d;
}

int dtls_seal(BSSL_AMD_DTLS_AEAD *t, const BSSL_AMD_DTLS_RECORDS *r, void *stream) {
  const uint64_t n = r->num_records;
  if (n == 0) return 1;
  // HasNext (dtls_record.cc:500-505): every record needs a number.
  if (t->seq > kDtlsMaxSequence || n - 1 > kDtlsMaxSequence - t->seq) {
    PUT_ERROR(ERR_R_OVERFLOW);
    return 0;
  }
  const KeyMaterial *km = state_of(&t->ctx)->km;
  if (!on_key_device(km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DtlsScratch sc(s, n, t->ad_stride(), false);
  if (!sc.buf) return 0;
  BatchDesc d = batch_desc(t, r, sc);
  DtlsPrepare p;
  fill_prepare(&p, t, r, sc);
  p.seq = t->seq;
  bool ok;
  Timed prepare(s);
  if (t->dtls13) {
    // The fragment is content || type, the layout of the TLS 1.3 padded seal
    // with no padding: its pre-pass writes the fragment lengths and flags and
    // puts the fragments in `out`, where the bulk kernel then runs in place.
    TlsPadSeal ps;
    memset(&ps, 0, sizeof(ps));
    ps.n = n;
    ps.in = r->in;
    ps.out = r->out;
    ps.offsets = r->offsets;
    ps.lengths = r->lengths;
    ps.record_stride = r->record_stride;
    ps.record_len = r->record_len;
    ps.types = r->types;
    ps.type = r->type;
    ps.frag_len = sc.frag_len;
    ps.out_lengths = r->out_lengths;
    ps.valid = sc.valid;
    ok = launch_tls13_pad_seal(ps, stream) == 0;
    p.lengths = sc.frag_len;
    d.in = r->out;
    d.lengths = sc.frag_len;
  } else {
    ok = hipMemsetAsync(sc.valid, 1, n, s) == hipSuccess;
    p.types = r->types;
    p.type = r->type;
    p.out_lengths = r->out_lengths;
  }
  ok = ok && launch_dtls_prepare(p, t->mask, stream) == 0;
  prepare.stop();
  secure_zero(&p, sizeof(p));
  ok = ok && launch_desc(km, d, false, stream) == 0;
  if (ok && t->dtls13) {
    Timed mask(s);
    const DtlsMaskSeal m = {n,           r->out,    r->offsets, sc.frag_len, r->record_stride,
                            r->record_len, r->prefix, r->suffix,  d.status,    t->state};
    ok = launch_dtls_mask(m, t->mask, stream) == 0;
    mask.stop();
  }
  if (ok) t->seq += n;
  return finish(ok);
}

int dtls_open(BSSL_AMD_DTLS_AEAD *t, const BSSL_AMD_DTLS_RECORDS *r, void *stream) {
  const uint64_t n = r->num_records;
  if (n == 0) return 1;
  const KeyMaterial *km = state_of(&t->ctx)->km;
  if (!on_key_device(km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DtlsScratch sc(s, n, t->ad_stride(), true);
  if (!sc.buf) return 0;
  BatchDesc d = batch_desc(t, r, sc);
  uint8_t *types = r->types ? r->types : sc.types;
  DtlsPrepare p;
  fill_prepare(&p, t, r, sc);
  p.body = r->in;
  p.types_out = t->dtls13 ? nullptr : r->types;
  p.ad_lengths = sc.ad_len;
  p.seqs = sc.seqs;
  Timed prepare(s);
  bool ok = launch_dtls_prepare(p, t->mask, stream) == 0;
  prepare.stop();
  secure_zero(&p, sizeof(p));
  if (t->dtls13) d.ad_lengths = sc.ad_len;  // the header as received: 2 to 5 bytes
  ok = ok && launch_desc(km, d, true, stream) == 0;
  if (ok && t->dtls13) {
    // The last non-zero byte of the fragment: the type, and the content length.
    Timed strip(s);
    const TlsPadStrip st = {n,        d.out, d.offsets,     d.lengths, d.record_stride, d.record_len,
                            d.status, types, r->out_lengths};
    ok = launch_tls13_pad_strip(st, stream) == 0;
    strip.stop();
  }
  if (ok) {
    Timed window(s);
    DtlsWindow w;
    memset(&w, 0, sizeof(w));
    w.n = n;
    w.out = r->out;
    w.offsets = r->offsets;
    w.lengths = r->lengths;
    w.record_stride = r->record_stride;
    w.record_len = r->record_len;
    w.status = d.status;
    w.out_lengths = r->out_lengths;
    w.set_lengths = !t->dtls13;
    w.types = t->dtls13 ? types : nullptr;
    w.seqs = sc.seqs;
    w.table = sc.table;
    w.table_slots = sc.table_slots;
    w.block_max = sc.block_max;
    w.old = sc.old;
    w.state = t->state;
    ok = launch_dtls_window(w, stream) == 0;
    window.stop();
  }
  return finish(ok);
}

}  // namespace

extern "C" {

BSSL_AMD_DTLS_AEAD *BSSL_AMD_DTLS_AEAD_new(enum evp_aead_direction_t direction, uint16_t version,
                                           const EVP_AEAD *aead, const uint8_t *key,
                                           size_t key_len, const uint8_t *fixed_iv,
                                           size_t fixed_iv_len, const uint8_t *sn_key,
                                           size_t sn_key_len, uint16_t epoch, uint64_t seq) {
  // All checks before any GPU call.  Epoch 0 of DTLS 1.3 is the plaintext
  // epoch (use_dtls13_record_header, dtls_record.cc:163-168).
  const bool dtls13 = version == BSSL_AMD_DTLS1_3_VERSION;
  if ((!dtls13 && version != BSSL_AMD_DTLS1_2_VERSION) || !aead || !key || !fixed_iv ||
      (dtls13 && epoch == 0) || seq > kDtlsMaxSequence) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return nullptr;
  }
  if (aead->kind == kAeadAesCtrHmac || aead->kind == kAeadTlsCbc) {  // as BSSL_AMD_TLS_AEAD_new
    PUT_ERROR(CIPHER_R_CTRL_NOT_IMPLEMENTED);
    return nullptr;
  }
  const bool chacha = aead == EVP_aead_chacha20_poly1305();
  const bool xor_nonce = dtls13 || chacha;
  if ((!chacha && aead != EVP_aead_aes_128_gcm() && aead != EVP_aead_aes_256_gcm()) ||
      key_len != aead->key_len || fixed_iv_len != (xor_nonce ? 12u : 4u) ||
      sn_key_len != (dtls13 ? aead->key_len : 0u)) {
    PUT_ERROR(CIPHER_R_UNSUPPORTED_KEY_SIZE);
    return nullptr;
  }
  if ((dtls13 && !sn_key) || (!dtls13 && sn_key)) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return nullptr;
  }
  BSSL_AMD_DTLS_AEAD *t = new (std::nothrow) bssl_amd_dtls_aead_st;
  if (!t) {
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  EVP_AEAD_CTX_zero(&t->ctx);
  if (!EVP_AEAD_CTX_init_with_direction(&t->ctx, aead, key, key_len, EVP_AEAD_DEFAULT_TAG_LENGTH,
                                        direction)) {
    delete t;
    return nullptr;
  }
  t->seal = direction == evp_aead_seal;
  t->dtls13 = dtls13;
  t->xor_nonce = xor_nonce;
  t->mask = !dtls13 ? kDtlsMaskNone
            : chacha ? kDtlsMaskChaCha
                     : aead->key_len == 16 ? kDtlsMaskAes128 : kDtlsMaskAes256;
  t->epoch = epoch;
  t->seq = seq;
  memset(t->fixed_iv, 0, sizeof(t->fixed_iv));
  memcpy(t->fixed_iv, fixed_iv, fixed_iv_len);
  t->state = nullptr;
  // The device state: an empty window at 0 and the record-number key, expanded
  // once (the kernels read it with scalar loads).
  DtlsState host;
  memset(&host, 0, sizeof(host));
  bool ok = mask_key_words(t->mask, sn_key, sn_key_len, host.sn);
  ok = ok && hipMalloc(reinterpret_cast<void **>(&t->state), sizeof(DtlsState)) == hipSuccess;
  if (!ok) t->state = nullptr;
  ok = ok && hipMemcpy(t->state, &host, sizeof(host), hipMemcpyHostToDevice) == hipSuccess;
  secure_zero(&host, sizeof(host));
  if (!ok) {
    BSSL_AMD_DTLS_AEAD_free(t);
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  return t;
}

void BSSL_AMD_DTLS_AEAD_free(BSSL_AMD_DTLS_AEAD *t) {
  if (!t) return;
  if (t->state) {
    DeviceGuard g(state_of(&t->ctx)->km->device);
    // As free_keys: drain the device, wipe, drain, free.
    hipDeviceSynchronize();
    hipMemset(t->state, 0, sizeof(DtlsState));
    hipDeviceSynchronize();
    hipFree(t->state);
  }
  EVP_AEAD_CTX_cleanup(&t->ctx);
  secure_zero(t->fixed_iv, sizeof(t->fixed_iv));
  delete t;
}

size_t BSSL_AMD_DTLS_AEAD_prefix_len(const BSSL_AMD_DTLS_AEAD *t) { return t->prefix_len(); }

uint64_t BSSL_AMD_DTLS_AEAD_sequence(const BSSL_AMD_DTLS_AEAD *t) { return t->seq; }

int BSSL_AMD_DTLS_AEAD_get_window(BSSL_AMD_DTLS_AEAD *t, uint64_t *max_seq, uint8_t bitmap[32],
                                  void *hip_stream) {
  if (!present(t) || !present(max_seq) || !present(bitmap)) return 0;
  if (!on_key_device(state_of(&t->ctx)->km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  uint64_t w[5];  // (little-endian host: bit k of the map is byte k / 8, bit k % 8)
  if (hipMemcpyAsync(w, t->state, sizeof(w), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return finish(false);
  *max_seq = w[0];
  memcpy(bitmap, w + 1, 32);
  return 1;
}

int BSSL_AMD_DTLS_AEAD_set_window(BSSL_AMD_DTLS_AEAD *t, uint64_t max_seq, const uint8_t bitmap[32],
                                  void *hip_stream) {
  if (!present(t) || !present(bitmap)) return 0;
  if (max_seq > kDtlsMaxSequence) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  if (!on_key_device(state_of(&t->ctx)->km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  uint64_t w[5];
  w[0] = max_seq;
  memcpy(w + 1, bitmap, 32);
  // (The copy reads this frame: wait until it has.)
  return finish(hipMemcpyAsync(t->state, w, sizeof(w), hipMemcpyHostToDevice, s) == hipSuccess &&
                hipStreamSynchronize(s) == hipSuccess);
}

int BSSL_AMD_DTLS_AEAD_seal_records_device(BSSL_AMD_DTLS_AEAD *t, const BSSL_AMD_DTLS_RECORDS *r,
                                           void *hip_stream) {
  return dtls_args_ok(t, r, true) ? dtls_seal(t, r, hip_stream) : 0;
}

int BSSL_AMD_DTLS_AEAD_open_records_device(BSSL_AMD_DTLS_AEAD *t, const BSSL_AMD_DTLS_RECORDS *r,
                                           void *hip_stream) {
  return dtls_args_ok(t, r, false) ? dtls_open(t, r, hip_stream) : 0;
}

}  // extern "C"
