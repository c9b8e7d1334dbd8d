// tls_api.cc -- the C ABI of include/bssl_amd/tls.h: the TLS record layer over
// device batches.
//
// SSLAEADContext (ssl/ssl_aead_ctx.cc) + do_seal_record / tls_open_record
// (ssl/tls_record.cc) for a batch of records; the per-record nonce, header,
// AD and inner type are built on the device (tls_records.hip, tls_set.hip) and
// the records go through the same bulk kernels as any batch (launch_desc).
// One connection with an AEAD suite, one connection with a CBC suite and a set
// of many connections differ in what they pass to the shared pieces below:
// TlsShape, TlsScratch, tls_fill_prepare, tls_batch_desc and tls_launch.  The
// TLS 1.3 padded calls are the same two paths with TlsShape::padded set: a
// pre-pass before a seal and a strip after an open (tls_pad.hip).
#include <hip/hip_runtime.h>
#include <errno.h>
#include <string.h>
#include <sys/random.h>

#include <new>
#include <vector>

#include "bssl_amd/tls.h"
#include "bssl_amd/test_hooks.h"
#include "set_api.h"

using namespace bssl_amd;

namespace {

// What a context or a set knows of its records' layout.
struct TlsShape {
  bool seal;
  bool tls13;
  bool xor_nonce;         // fixed IV XOR seq (TLS 1.3, TLS 1.2 ChaCha) vs fixed || seq
  uint32_t explicit_len;  // 8: TLS 1.2 AES-GCM's explicit nonce; 16: a CBC suite's IV; else 0
  // The TLS 1.3 padded calls (never set in a context's or a set's own shape):
  // the body is the whole fragment, type and zeros included, so there is no
  // extra byte, the suffix is the tag alone and the header length comes from
  // the fragment length (tls_pad.hip).
  bool padded = false;
  uint32_t ad_stride() const { return tls13 ? 5 : 13; }
  uint32_t extra_len() const { return tls13 && !padded ? 1 : 0; }  // the inner content type
  uint32_t prefix_len() const { return 5 + explicit_len; }
  uint32_t suffix_len(uint32_t tag_len) const { return extra_len() + tag_len; }
  // TLS 1.2 open reports the header type (tls_record.cc:197-235): where to.
  uint8_t *header_types(const BSSL_AMD_TLS_RECORDS *r) const {
    return !seal && !tls13 ? r->types : nullptr;
  }
  // The shape of a padded call, or false (error queued) when the context or
  // set is not TLS 1.3 -- a CBC context's shape never is.
  bool padded_form(TlsShape *out) const {
    if (!tls13) {
      PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
      return false;
    }
    *out = *this;
    out->padded = true;
    return true;
  }
};

const EVP_AEAD *tls_record_aead(const EVP_AEAD *aead, bool tls13) {
  // ssl_cipher_get_evp_aead (ssl/ssl_cipher.cc): the nonce-checking variants
  // for AES-GCM in TLS 1.2 / 1.3.
  if (aead == EVP_aead_aes_128_gcm())
    return tls13 ? EVP_aead_aes_128_gcm_tls13() : EVP_aead_aes_128_gcm_tls12();
  if (aead == EVP_aead_aes_256_gcm())
    return tls13 ? EVP_aead_aes_256_gcm_tls13() : EVP_aead_aes_256_gcm_tls12();
  if (aead == EVP_aead_chacha20_poly1305()) return aead;
  return nullptr;
}

// SSLAEADContext::Create (ssl_aead_ctx.cc:44-123) for an AEAD suite: checks
// (version, aead) -- all before any GPU call -- and fills the shape.  args_ok:
// the caller's own null / range checks, which share the first code.  Returns
// the AEAD of the records (tls_record_aead), or null with the error queued.
const EVP_AEAD *tls_shape_init(TlsShape *sh, enum evp_aead_direction_t direction, uint16_t version,
                               const EVP_AEAD *aead, bool args_ok) {
  if ((version != BSSL_AMD_TLS1_2_VERSION && version != BSSL_AMD_TLS1_3_VERSION) || !aead ||
      !args_ok) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return nullptr;
  }
  if (aead->kind == kAeadAesCtrHmac || aead->kind == kAeadTlsCbc) {  // no record layer for them here (tls.h)
    PUT_ERROR(CIPHER_R_CTRL_NOT_IMPLEMENTED);
    return nullptr;
  }
  sh->seal = direction == evp_aead_seal;
  sh->tls13 = version == BSSL_AMD_TLS1_3_VERSION;
  const EVP_AEAD *rec_aead = tls_record_aead(aead, sh->tls13);
  if (!rec_aead) {
    PUT_ERROR(CIPHER_R_UNSUPPORTED_KEY_SIZE);
    return nullptr;
  }
  // TLS 1.3 and TLS 1.2 ChaCha20-Poly1305 XOR a 12-byte IV with the sequence
  // number; TLS 1.2 AES-GCM prepends a 4-byte IV to an 8-byte explicit nonce.
  sh->xor_nonce = sh->tls13 || aead->kind == kAeadChaChaPoly;
  sh->explicit_len = sh->xor_nonce ? 0 : 8;
  return rec_aead;
}

// The scratch of one call (one stream-ordered block, freed in stream order on
// every path: CallScratch, set_api.h): per record a padded call's fragment
// length and the set's key index (both first: alignment; null without), the
// nonce, the AD, the inner type (seal, TLS 1.3; type_len 0: none), the flag,
// and a padded call's status byte for a caller who passes none (else null).
struct TlsLayout {
  uint64_t n;
  uint32_t nonce_len, ad_stride, type_len;
  bool keys, padded;
  uint64_t *frag_len;
  uint32_t *key_index;
  uint8_t *nonce, *ad, *type, *valid, *status;
  TlsLayout(uint64_t records, uint32_t nonce_bytes, uint32_t ad_bytes, uint32_t type_bytes,
            bool key_indices, bool is_padded = false)
      : n(records), nonce_len(nonce_bytes), ad_stride(ad_bytes), type_len(type_bytes),
        keys(key_indices), padded(is_padded) {}
  void carve(Carver &c) {
    frag_len = padded ? c.take<uint64_t>(n) : nullptr;
    key_index = keys ? c.take<uint32_t>(n) : nullptr;
    nonce = c.take<uint8_t>(nonce_len * n);
    ad = c.take<uint8_t>(ad_stride * n);
    type = c.take<uint8_t>(type_len * n);
    valid = c.take<uint8_t>(n);
    status = padded ? c.take<uint8_t>(n) : nullptr;
  }
};
using TlsScratch = CallScratch<TlsLayout>;

// The prepare step's inputs of an AEAD suite's batch, all but fixed_iv and seq
// (one connection adds them; a set's come from its connections).
void tls_fill_prepare(TlsPrepare *p, const TlsShape &sh, const BSSL_AMD_TLS_RECORDS *r,
                      const TlsScratch &sc, uint32_t tag_len) {
  memset(p, 0, sizeof(*p));
  p->n = r->num_records;
  // (A padded seal's lengths are the pre-pass's fragment lengths.)
  p->lengths = sh.padded && sh.seal ? sc.frag_len : r->lengths;
  p->record_len = r->record_len;
  p->types = r->types;
  p->type = r->type;
  p->padded = sh.padded;
  p->out_lengths = sh.padded && sh.seal ? r->out_lengths : nullptr;
  p->xor_nonce = sh.xor_nonce;
  p->tls13 = sh.tls13;
  p->record_version = 0x0303;  // tls_record_version: TLS 1.3 records say TLS 1.2
  p->explicit_len = sh.explicit_len;
  p->extra_len = sh.extra_len();
  p->tag_len = tag_len;
  p->prefix_len = sh.prefix_len();
  p->ad_stride = sh.ad_stride();
  p->open = !sh.seal;
  p->nonces = sc.nonce;
  p->prefix = r->prefix;
  p->ad = sc.ad;
  p->extra = sc.type;
  p->valid = sc.valid;
}

// The bulk kernels' descriptor of a record-layer batch: the bodies where the
// caller has them, nonces (nonce_len bytes), ADs (ad_len bytes) and flags in
// the scratch, the tags in the suffix slots after the sealed inner type.  One
// key; a set adds key_index / num_keys, CBC open out_lengths / max_plain_len.
// A padded seal runs in place on `out`, where the pre-pass has put the
// fragments, over the fragment lengths in the scratch; a padded open always
// has a status array, for the strip that follows.
BatchDesc tls_batch_desc(const BSSL_AMD_TLS_RECORDS *r, const TlsScratch &sc, uint32_t nonce_len,
                         uint32_t ad_len, uint32_t tag_len, const TlsShape &sh) {
  const uint32_t extra_len = sh.extra_len(), suffix_len = sh.suffix_len(tag_len);
  BatchDesc d;
  memset(&d, 0, sizeof(d));
  d.in = r->in;
  d.out = r->out;
  d.offsets = r->offsets;
  d.lengths = r->lengths;
  d.record_stride = r->record_stride;
  d.record_len = r->record_len;
  d.nonces = sc.nonce;
  d.nonce_len = nonce_len;
  d.ad = sc.ad;
  d.ad_stride = ad_len;
  d.ad_len = ad_len;
  d.tags = r->suffix + extra_len;
  d.tag_stride = suffix_len;
  d.status = r->status;
  d.num_records = r->num_records;
  d.tag_len = tag_len;
  d.num_keys = 1;
  d.valid = sc.valid;
  if (sh.padded && sh.seal) {
    d.in = r->out;
    d.lengths = sc.frag_len;
  }
  if (sh.padded && !sh.seal && !d.status) d.status = sc.status;
  if (extra_len) {
    d.extra_len = extra_len;
    if (sh.seal) {  // inner type in, its ciphertext to the suffix
      d.extra = sc.type;
      d.extra_stride = 1;
      d.extra_out = r->suffix;
      d.extra_out_stride = suffix_len;
    } else {        // sealed inner type from the suffix, plaintext type out
      d.extra = r->suffix;
      d.extra_stride = suffix_len;
      d.extra_out = r->types;
      d.extra_out_stride = 1;
    }
  }
  return d;
}

// The end of every call: the bulk kernels (when the steps before were `ok`),
// the header types of a TLS 1.2 AEAD-suite open (or null), a padded open's
// strip into types / out_lengths, the error; *seq (one connection, or null)
// advances only on success.  Returns 1 or 0.
int tls_launch(bool ok, const KeyMaterial *km, const BatchDesc &d, const TlsShape &sh,
               uint8_t *header_types, const BSSL_AMD_TLS_RECORDS *r, uint64_t *seq,
               void *stream) {
  const uint8_t *prefix = r->prefix;
  ok = ok && launch_desc(km, d, !sh.seal, stream) == 0;
  if (ok && sh.padded && !sh.seal) {
    const TlsPadStrip strip = {d.num_records, d.out,    d.offsets, d.lengths,     d.record_stride,
                               d.record_len,  d.status, r->types,  r->out_lengths};
    ok = launch_tls13_pad_strip(strip, stream) == 0;
  }
  if (ok && header_types)
    ok = hipMemcpy2DAsync(header_types, 1, prefix, sh.prefix_len(), 1, d.num_records,
                          hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream)) == hipSuccess;
  if (!ok) {
    PUT_ERROR(ERR_R_INTERNAL_ERROR);
    return 0;
  }
  if (seq) *seq += d.num_records;
  return 1;
}

// The null checks of a batch, and for a padded open the two outputs it exists
// for.  False with the error queued.
bool tls_records_args_ok(const BSSL_AMD_TLS_RECORDS *r, const TlsShape &sh) {
  if (r && (r->num_records == 0 ||
            (r->in && r->out && r->prefix && r->suffix &&
             !(sh.padded && !sh.seal && (!r->out_lengths || !r->types)))))
    return true;
  PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
  return false;
}

// A padded seal's pre-pass (tls_pad.hip): fragment lengths and flags into the
// scratch, the type bytes and zeros behind the contents in `out`.
bool tls_pad_seal(const BSSL_AMD_TLS_RECORDS *r, const BSSL_AMD_TLS13_PADDING *pad,
                  const TlsScratch &sc, void *stream) {
  TlsPadSeal p;
  memset(&p, 0, sizeof(p));
  p.n = r->num_records;
  p.in = r->in;
  p.out = r->out;
  p.offsets = r->offsets;
  p.lengths = r->lengths;
  p.record_stride = r->record_stride;
  p.record_len = r->record_len;
  p.types = r->types;
  p.type = r->type;
  p.pad_lengths = pad ? pad->pad_lengths : nullptr;
  p.pad_block = pad ? pad->pad_block : 0;
  p.frag_len = sc.frag_len;
  p.out_lengths = r->out_lengths;
  p.valid = sc.valid;
  return launch_tls13_pad_seal(p, stream) == 0;
}

}  // namespace

// ---- One connection (BSSL_AMD_TLS_AEAD) ------------------------------------

struct bssl_amd_tls_aead_st {
  EVP_AEAD_CTX ctx;
  TlsShape shape;
  uint8_t fixed_iv[12];
  uint64_t seq;
  // The CBC suites (BSSL_AMD_TLS_AEAD_new_cbc): the record version, and for a
  // sealing context the key of the IV generator (tls_records.hip).
  bool cbc;
  uint16_t version;
  uint8_t iv_key[32];
};

namespace {

// The CBC suites: random_variable_nonce_ / omit_length_in_ad_ of
// SSLAEADContext (ssl_aead_ctx.cc:109-113) and the limits of tls_open_record
// (tls_record.cc:117-133, 204-209).
int tls_cbc_records(BSSL_AMD_TLS_AEAD *t, const BSSL_AMD_TLS_RECORDS *r, void *stream) {
  const TlsShape &sh = t->shape;
  // Open takes whole fragments (no suffix) and must report the lengths.
  if (!r || (r->num_records && (!r->in || !r->out || !r->prefix ||
                                (sh.seal ? !r->suffix : !r->out_lengths)))) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  const uint64_t n = r->num_records;
  if (n == 0) return 1;
  if (t->seq > UINT64_MAX - n) {
    PUT_ERROR(ERR_R_OVERFLOW);
    return 0;
  }
  const KeyMaterial *km = state_of(&t->ctx)->km;
  if (!on_key_device(km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // Scratch: IVs (16 B), AD (11 B) and flags per record.
  TlsScratch sc(s, n, 16, 11, 0, false);
  if (!sc.buf) return 0;
  bool ok = hipMemsetAsync(sc.valid, 1, n, s) == hipSuccess;
  TlsCbcPrepare p;
  memset(&p, 0, sizeof(p));
  p.n = n;
  p.lengths = r->lengths;
  p.record_len = r->record_len;
  p.types = sh.seal ? r->types : nullptr;
  p.type = r->type;
  p.record_version = t->version;
  p.mac_len = (uint32_t)tls_cbc_mac_len(t->ctx.aead);
  p.seq = t->seq;
  p.open = !sh.seal;
  p.explicit_ivs = sh.seal ? r->explicit_ivs : nullptr;
  if (sh.seal) memcpy(p.iv_key, t->iv_key, sizeof(p.iv_key));  // (little-endian host)
  p.nonces = sc.nonce;
  p.prefix = r->prefix;
  p.ad = sc.ad;
  p.valid = sc.valid;
  p.types_out = sh.seal ? nullptr : r->types;
  ok = ok && launch_tls_cbc_prepare(p, stream) == 0;
  secure_zero(&p, sizeof(p));
  // The suffix as tag slots of the overhead: the MAC and the longest padding.
  BatchDesc d = tls_batch_desc(r, sc, 16, 11, t->ctx.aead->overhead, sh);
  if (!sh.seal) {
    d.out_lengths = r->out_lengths;
    d.max_plain_len = kTlsMaxPlainLen;
  }
  // (No header types to copy: on open the prepare kernel wrote them, types_out.)
  return tls_launch(ok, km, d, sh, nullptr, r, &t->seq, stream);
}

// `sh`: the context's shape, or its padded form (then with `pad` on seal).
int tls_records(BSSL_AMD_TLS_AEAD *t, const TlsShape &sh, const BSSL_AMD_TLS_RECORDS *r,
                const BSSL_AMD_TLS13_PADDING *pad, void *stream) {
  if (!tls_records_args_ok(r, sh)) return 0;
  const uint64_t n = r->num_records;
  if (n == 0) return 1;
  // tls_record.cc:305-308: the sequence number must not wrap.
  if (t->seq > UINT64_MAX - n) {
    PUT_ERROR(ERR_R_OVERFLOW);
    return 0;
  }
  if (!sh.seal && sh.tls13 && !r->types) {  // open returns the inner types
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  const EVP_AEAD_CTX *ctx = &t->ctx;
  CtxState *st = state_of(ctx);
  if (!on_key_device(st->km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t tag_len = ctx->tag_len;
  // Scratch: nonces (12 B), AD, inner types (seal, TLS 1.3) and flags per record.
  TlsScratch sc(s, n, 12, sh.ad_stride(), 1, false, sh.padded);
  if (!sc.buf) return 0;
  // The flags start at 1, or for a padded seal as its pre-pass leaves them.
  bool ok = sh.padded && sh.seal ? tls_pad_seal(r, pad, sc, stream)
                                 : hipMemsetAsync(sc.valid, 1, n, s) == hipSuccess;
  TlsPrepare p;
  tls_fill_prepare(&p, sh, r, sc, tag_len);
  memcpy(p.fixed_iv, t->fixed_iv, 12);
  p.seq = t->seq;
  ok = ok && launch_tls_prepare(p, stream) == 0;
  if (ok && sh.seal && ctx->aead->tls)  // the AEAD's own nonce check (sealv)
    ok = tls_nonce_scan(sc.nonce, n, ctx->aead->tls, &st->min_next_nonce, &st->mask, sc.valid, 1,
                        stream) == 0;
  return tls_launch(ok, st->km, tls_batch_desc(r, sc, 12, sh.ad_stride(), tag_len, sh), sh,
                    sh.header_types(r), r, &t->seq, stream);
}

}  // namespace

extern "C" {

BSSL_AMD_TLS_AEAD *BSSL_AMD_TLS_AEAD_new(enum evp_aead_direction_t direction, uint16_t version,
                                         const EVP_AEAD *aead, const uint8_t *key,
                                         size_t key_len, const uint8_t *fixed_iv,
                                         size_t fixed_iv_len, uint64_t seq) {
  TlsShape sh;
  const EVP_AEAD *rec_aead = tls_shape_init(&sh, direction, version, aead, fixed_iv != nullptr);
  if (!rec_aead) return nullptr;
  if (fixed_iv_len != (sh.xor_nonce ? 12u : 4u)) {
    PUT_ERROR(CIPHER_R_INVALID_NONCE_SIZE);
    return nullptr;
  }
  BSSL_AMD_TLS_AEAD *t = new (std::nothrow) bssl_amd_tls_aead_st;
  if (!t) {
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  EVP_AEAD_CTX_zero(&t->ctx);
  if (!EVP_AEAD_CTX_init_with_direction(&t->ctx, rec_aead, key, key_len,
                                        EVP_AEAD_DEFAULT_TAG_LENGTH, direction)) {
    delete t;
    return nullptr;
  }
  t->shape = sh;
  memset(t->fixed_iv, 0, sizeof(t->fixed_iv));
  memcpy(t->fixed_iv, fixed_iv, fixed_iv_len);
  t->seq = seq;
  t->cbc = false;
  t->version = 0x0303;
  memset(t->iv_key, 0, sizeof(t->iv_key));
  if (sh.seal && sh.tls13 && t->ctx.aead->tls == 13 && seq != 0) {
    // The tls13 AEAD takes its nonce mask from the first sealed nonce, which
    // it assumes is sequence number 0 (e_aes.cc.inc:1181-1185).  A writer
    // that starts mid-stream gets the state the AEAD would have after
    // sealing records 0 .. seq-1: mask = the IV's low 64 bits, next >= seq.
    CtxState *st = state_of(&t->ctx);
    st->mask = load_be64(t->fixed_iv + 4);
    st->min_next_nonce = seq;
  }
  return t;
}

BSSL_AMD_TLS_AEAD *BSSL_AMD_TLS_AEAD_new_cbc(enum evp_aead_direction_t direction, uint16_t version,
                                             const EVP_AEAD *aead, const uint8_t *enc_key,
                                             size_t enc_key_len, const uint8_t *mac_key,
                                             size_t mac_key_len, uint64_t seq) {
  // SSLAEADContext::Create (ssl_aead_ctx.cc:95-114) for a CBC suite with an
  // explicit IV: TLS 1.1 and 1.2, no fixed IV.
  if ((version != BSSL_AMD_TLS1_1_VERSION && version != BSSL_AMD_TLS1_2_VERSION) || !aead ||
      !enc_key || !mac_key) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return nullptr;
  }
  if (aead->kind != kAeadTlsCbc) {
    PUT_ERROR(CIPHER_R_CTRL_NOT_IMPLEMENTED);
    return nullptr;
  }
  if (mac_key_len != tls_cbc_mac_len(aead) || mac_key_len + enc_key_len != aead->key_len) {
    PUT_ERROR(CIPHER_R_UNSUPPORTED_KEY_SIZE);
    return nullptr;
  }
  BSSL_AMD_TLS_AEAD *t = new (std::nothrow) bssl_amd_tls_aead_st;
  if (!t) {
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  memset(t->iv_key, 0, sizeof(t->iv_key));
  t->shape = TlsShape{direction == evp_aead_seal, false, false, 16};
  if (t->shape.seal) {
    // The IV generator's key (RAND_bytes per record in the reference,
    // ssl_aead_ctx.cc:343-347).
    size_t got = 0;
    while (got < sizeof(t->iv_key)) {
      const ssize_t k = getrandom(t->iv_key + got, sizeof(t->iv_key) - got, 0);
      if (k < 0 && errno == EINTR) continue;
      if (k <= 0) break;
      got += (size_t)k;
    }
    if (got != sizeof(t->iv_key)) {
      secure_zero(t->iv_key, sizeof(t->iv_key));
      delete t;
      PUT_ERROR(ERR_R_INTERNAL_ERROR);
      return nullptr;
    }
  }
  uint8_t merged[64];  // MAC key || AES key, at most 52 bytes
  memcpy(merged, mac_key, mac_key_len);
  memcpy(merged + mac_key_len, enc_key, enc_key_len);
  EVP_AEAD_CTX_zero(&t->ctx);
  const int ok = EVP_AEAD_CTX_init_with_direction(&t->ctx, aead, merged, mac_key_len + enc_key_len,
                                                  EVP_AEAD_DEFAULT_TAG_LENGTH, direction);
  secure_zero(merged, sizeof(merged));
  if (!ok) {
    secure_zero(t->iv_key, sizeof(t->iv_key));
    delete t;
    return nullptr;
  }
  memset(t->fixed_iv, 0, sizeof(t->fixed_iv));
  t->seq = seq;
  t->cbc = true;
  t->version = version;
  return t;
}

void BSSL_AMD_TLS_AEAD_free(BSSL_AMD_TLS_AEAD *t) {
  if (!t) return;
  EVP_AEAD_CTX_cleanup(&t->ctx);
  secure_zero(t->iv_key, sizeof(t->iv_key));
  delete t;
}

int BSSL_AMD_test_tls_set_iv_key(BSSL_AMD_TLS_AEAD *t, const uint8_t key[32]) {
  if (!t || !t->cbc || !t->shape.seal || !key) return 0;
  memcpy(t->iv_key, key, sizeof(t->iv_key));
  return 1;
}

size_t BSSL_AMD_TLS_AEAD_prefix_len(const BSSL_AMD_TLS_AEAD *t) { return t->shape.prefix_len(); }

size_t BSSL_AMD_TLS_AEAD_suffix_len(const BSSL_AMD_TLS_AEAD *t) {
  // CBC: the tag slot, the MAC and the longest padding.
  return t->shape.suffix_len(t->cbc ? t->ctx.aead->overhead : t->ctx.tag_len);
}

uint64_t BSSL_AMD_TLS_AEAD_sequence(const BSSL_AMD_TLS_AEAD *t) { return t->seq; }

int BSSL_AMD_TLS_AEAD_seal_records_device(BSSL_AMD_TLS_AEAD *t, const BSSL_AMD_TLS_RECORDS *r,
                                          void *hip_stream) {
  if (!present(t) || !direction_ok(t->shape.seal, true)) return 0;
  return t->cbc ? tls_cbc_records(t, r, hip_stream)
                : tls_records(t, t->shape, r, nullptr, hip_stream);
}

int BSSL_AMD_TLS_AEAD_open_records_device(BSSL_AMD_TLS_AEAD *t, const BSSL_AMD_TLS_RECORDS *r,
                                          void *hip_stream) {
  if (!present(t) || !direction_ok(t->shape.seal, false)) return 0;
  return t->cbc ? tls_cbc_records(t, r, hip_stream)
                : tls_records(t, t->shape, r, nullptr, hip_stream);
}

int BSSL_AMD_TLS_AEAD_seal_tls13_padded_device(BSSL_AMD_TLS_AEAD *t, const BSSL_AMD_TLS_RECORDS *r,
                                               const BSSL_AMD_TLS13_PADDING *pad,
                                               void *hip_stream) {
  TlsShape sh;
  if (!present(t) || !t->shape.padded_form(&sh) || !direction_ok(sh.seal, true)) return 0;
  return tls_records(t, sh, r, pad, hip_stream);
}

int BSSL_AMD_TLS_AEAD_open_tls13_padded_device(BSSL_AMD_TLS_AEAD *t, const BSSL_AMD_TLS_RECORDS *r,
                                               void *hip_stream) {
  TlsShape sh;
  if (!present(t) || !t->shape.padded_form(&sh) || !direction_ok(sh.seal, false)) return 0;
  return tls_records(t, sh, r, nullptr, hip_stream);
}

}  // extern "C"

// ---- Connection sets (BSSL_AMD_TLS_SET) ------------------------------------
// One direction of many connections of one cipher suite: a keyset plus the
// per-connection fixed IVs and sequence numbers on the device (TlsSetConn,
// tls_set.hip), so that a mixed batch of records is one call that only
// enqueues work.  The AEAD is the plain one (keysets have no per-key nonce
// state): nothing but the set advances a connection's counter, so its nonces
// increase by construction.

struct bssl_amd_tls_set_st {
  KeyMaterial *km;    // the keyset: num_connections keys, zero until installed
  TlsSetConn *conns;  // device, num_connections entries
  TlsShape shape;
};

namespace {

constexpr uint32_t kSetTagLen = 16;

// `sh`: the set's shape, or its padded form (then with `pad` on seal).
int tls_set_records(BSSL_AMD_TLS_SET *t, const TlsShape &sh, const BSSL_AMD_TLS_SET_RECORDS *sr,
                    const BSSL_AMD_TLS13_PADDING *pad, void *stream) {
  const BSSL_AMD_TLS_RECORDS *r = sr ? &sr->records : nullptr;
  if (!tls_records_args_ok(r, sh)) return 0;
  if ((r->num_records && (sr->num_runs == 0 || !sr->run_connection || !sr->run_start)) ||
      sr->num_runs > 0xfffffffeu) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  const uint64_t n = r->num_records;
  if (n == 0) return 1;
  if (!sh.seal && sh.tls13 && !r->types) {  // open returns the inner types
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  const KeyMaterial *km = t->km;
  if (!on_key_device(km)) return 0;
  // Scratch per record: the key index, the nonce (12 B), the AD, the inner
  // type (seal, TLS 1.3) and the flag (tls_set_prepare_kernel writes every one).
  TlsScratch sc(reinterpret_cast<hipStream_t>(stream), n, 12, sh.ad_stride(), 1, true, sh.padded);
  if (!sc.buf) return 0;
  bool ok = !(sh.padded && sh.seal) || tls_pad_seal(r, pad, sc, stream);
  TlsSetPrepare p;
  memset(&p, 0, sizeof(p));
  tls_fill_prepare(&p.rec, sh, r, sc, kSetTagLen);
  p.conns = t->conns;
  // (No flag, run_of or run_won: the TLS frame is the lax one, set_runs.h.)
  p.runs = {(uint32_t)km->num_keys, sr->num_runs, sr->run_connection, sr->run_start,
            sc.key_index,           nullptr,      nullptr,            nullptr};
  ok = ok && launch_tls_set_prepare(p, stream) == 0;
  BatchDesc d = tls_batch_desc(r, sc, 12, sh.ad_stride(), kSetTagLen, sh);
  d.key_index = sc.key_index;
  d.num_keys = (uint32_t)km->num_keys;
  return tls_launch(ok, km, d, sh, sh.header_types(r), r, nullptr, stream);
}

}  // namespace

extern "C" {

BSSL_AMD_TLS_SET *BSSL_AMD_TLS_SET_new(enum evp_aead_direction_t direction, uint16_t version,
                                       const EVP_AEAD *aead, size_t num_connections) {
  // The rules and codes of BSSL_AMD_TLS_AEAD_new, all before any GPU call.
  TlsShape sh;
  if (!tls_shape_init(&sh, direction, version, aead,
                      num_connections != 0 && num_connections <= 0xfffffffeu))
    return nullptr;
  BSSL_AMD_TLS_SET *t = new (std::nothrow) bssl_amd_tls_set_st;
  if (t)
    t->km = keyset_new(aead, num_connections, sizeof(TlsSetConn),
                       reinterpret_cast<void **>(&t->conns));
  if (!t || !t->km) {
    delete t;
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  t->shape = sh;
  return t;
}

void BSSL_AMD_TLS_SET_free(BSSL_AMD_TLS_SET *s) {
  if (!s) return;
  keyset_free(s->km, s->conns, sizeof(TlsSetConn));
  delete s;
}

size_t BSSL_AMD_TLS_SET_num_connections(const BSSL_AMD_TLS_SET *s) {
  return s ? s->km->num_keys : 0;
}

size_t BSSL_AMD_TLS_SET_prefix_len(const BSSL_AMD_TLS_SET *s) { return s->shape.prefix_len(); }

size_t BSSL_AMD_TLS_SET_suffix_len(const BSSL_AMD_TLS_SET *s) {
  return s->shape.suffix_len(kSetTagLen);
}

int BSSL_AMD_TLS_SET_set_connections(BSSL_AMD_TLS_SET *s, size_t first, size_t n,
                                     const uint8_t *keys, const uint8_t *fixed_ivs,
                                     const uint64_t *seqs, void *hip_stream) {
  if (!range_ok(s, first, n)) return 0;
  if (n == 0) return 1;
  if (!keys || !fixed_ivs) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  KeyMaterial *km = s->km;
  if (!on_key_device(km)) return 0;
  const size_t iv_len = s->shape.xor_nonce ? 12 : 4;
  // The connection state staged in host memory, wiped on every path once the
  // copy has read it.
  std::vector<TlsSetConn> host_conns(n);
  Wiped wipe{host_conns.data(), n * sizeof(TlsSetConn)};
  for (size_t i = 0; i < n; i++) {
    TlsSetConn &c = host_conns[i];
    memset(&c, 0, sizeof(c));
    c.seq = seqs ? seqs[i] : 0;
    pack_iv(fixed_ivs + i * iv_len, iv_len, &c.iv_lo, &c.iv_hi);
    c.live = 1;
  }
  return finish(install_slots(km, s->conns, sizeof(TlsSetConn), first, n, keys, host_conns.data(),
                              reinterpret_cast<hipStream_t>(hip_stream)));
}

int BSSL_AMD_TLS_SET_clear_connections(BSSL_AMD_TLS_SET *s, size_t first, size_t n,
                                       void *hip_stream) {
  if (!range_ok(s, first, n)) return 0;
  if (n == 0) return 1;
  if (!on_key_device(s->km)) return 0;
  return finish(clear_slots(s->km, s->conns, sizeof(TlsSetConn), first, n,
                            reinterpret_cast<hipStream_t>(hip_stream)));
}

int BSSL_AMD_TLS_SET_sequences(BSSL_AMD_TLS_SET *s, size_t first, size_t n, uint64_t *out,
                               void *hip_stream) {
  if (!range_ok(s, first, n)) return 0;
  if (n == 0) return 1;
  if (!out) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  if (!on_key_device(s->km)) return 0;
  const bool ok = copy_columns(s->conns, sizeof(TlsSetConn), first, n, offsetof(TlsSetConn, seq), 8,
                               out, true, reinterpret_cast<hipStream_t>(hip_stream));
  if (!ok) memset(out, 0, n * sizeof(uint64_t));
  return finish(ok);
}

int BSSL_AMD_TLS_SET_seal_records_device(BSSL_AMD_TLS_SET *s, const BSSL_AMD_TLS_SET_RECORDS *r,
                                         void *hip_stream) {
  if (!present(s) || !direction_ok(s->shape.seal, true)) return 0;
  return tls_set_records(s, s->shape, r, nullptr, hip_stream);
}

int BSSL_AMD_TLS_SET_open_records_device(BSSL_AMD_TLS_SET *s, const BSSL_AMD_TLS_SET_RECORDS *r,
                                         void *hip_stream) {
  if (!present(s) || !direction_ok(s->shape.seal, false)) return 0;
  return tls_set_records(s, s->shape, r, nullptr, hip_stream);
}

int BSSL_AMD_TLS_SET_seal_tls13_padded_device(BSSL_AMD_TLS_SET *s, const BSSL_AMD_TLS_SET_RECORDS *r,
                                              const BSSL_AMD_TLS13_PADDING *pad, void *hip_stream) {
  TlsShape sh;
  if (!present(s) || !s->shape.padded_form(&sh) || !direction_ok(sh.seal, true)) return 0;
  return tls_set_records(s, sh, r, pad, hip_stream);
}

int BSSL_AMD_TLS_SET_open_tls13_padded_device(BSSL_AMD_TLS_SET *s, const BSSL_AMD_TLS_SET_RECORDS *r,
                                              void *hip_stream) {
  TlsShape sh;
  if (!present(s) || !s->shape.padded_form(&sh) || !direction_ok(sh.seal, false)) return 0;
  return tls_set_records(s, sh, r, nullptr, hip_stream);
}

}  // extern "C"
