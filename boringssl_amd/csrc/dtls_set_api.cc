// dtls_set_api.cc -- the C ABI of BSSL_AMD_DTLS_SET (include/bssl_amd/tls.h):
// one direction of many DTLS 1.2 / 1.3 associations over device batches.
//
// What BSSL_AMD_DTLS_AEAD (dtls_api.cc) is for one association and
// BSSL_AMD_TLS_SET (tls_api.cc) for many TLS connections, composed: a keyset
// plus one DtlsSetSlot per slot on the device -- fixed IV, epoch, record-number
// key, write sequence number, replay window -- so that a batch that mixes the
// records of many associations is one call that only enqueues work: the
// claim / prepare / advance launches of dtls_set.hip, the bulk kernels of the
// AEAD with a key index per record (launch_desc), then on seal the DTLS 1.3
// record-number mask, on open the DTLS 1.3 strip (tls_pad.hip) and the
// per-slot replay windows.  The keyset, the slot array and the scratch block
// are set_api.h's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <vector>

#include "bssl_amd/tls.h"
#include "set_api.h"

using namespace bssl_amd;

struct bssl_amd_dtls_set_st {
  KeyMaterial *km;     // the keyset: num_slots keys, zero until installed
  DtlsSetSlot *slots;  // device, num_slots entries
  bool seal;
  bool dtls13;
  bool xor_nonce;  // fixed IV XOR the sequence number vs 4-byte IV || explicit nonce
  int mask;        // DtlsMask
  uint32_t prefix_len() const { return dtls13 ? 5 : xor_nonce ? 13 : 21; }
  uint32_t ad_stride() const { return dtls13 ? 5 : 13; }
};

namespace {

constexpr uint32_t kTagLen = 16;
constexpr size_t kMaxCount = 0xfffffffeu;  // slots, runs and records of a call

using Scratch = CallScratch<DtlsSetLayout>;

// The checks both record calls share; false with the error queued.
bool set_args_ok(const BSSL_AMD_DTLS_SET *t, const BSSL_AMD_DTLS_SET_RECORDS *sr, bool want_seal) {
  if (!present(t) || !direction_ok(t->seal, want_seal)) return false;
  if (!sr) return fail(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
  const BSSL_AMD_DTLS_RECORDS *r = &sr->records;
  if (r->num_records == 0) return true;
  if (r->in && r->out && r->prefix && r->suffix && !(!want_seal && t->dtls13 && !r->out_lengths) &&
      sr->num_runs != 0 && sr->run_slot && sr->run_start && sr->num_runs <= kMaxCount &&
      r->num_records <= kMaxCount)
    return true;
  return fail(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
}

void fill_prepare(DtlsSetPrepare *p, const BSSL_AMD_DTLS_SET *t, const BSSL_AMD_DTLS_SET_RECORDS *sr,
                  const Scratch &sc) {
  const BSSL_AMD_DTLS_RECORDS *r = &sr->records;
  memset(p, 0, sizeof(*p));
  p->rec.n = r->num_records;
  p->rec.offsets = r->offsets;
  p->rec.lengths = r->lengths;
  p->rec.record_stride = r->record_stride;
  p->rec.record_len = r->record_len;
  p->rec.open = !t->seal;
  p->rec.dtls13 = t->dtls13;
  p->rec.xor_nonce = t->xor_nonce;
  p->rec.prefix_len = t->prefix_len();
  p->rec.ad_stride = t->ad_stride();
  p->rec.prefix = r->prefix;
  p->rec.suffix = r->suffix;
  p->rec.nonces = sc.nonce;
  p->rec.ad = sc.ad;
  p->rec.valid = sc.valid;
  p->rec.record_numbers = r->record_numbers;
  p->slots = t->slots;
  p->runs = {(uint32_t)t->km->num_keys, sr->num_runs, sr->run_slot, sr->run_start,
             sc.key_index,              sc.flag,      sc.run_of,    sc.run_won};
}

BatchDesc batch_desc(const BSSL_AMD_DTLS_SET *t, const BSSL_AMD_DTLS_RECORDS *r,
                     const Scratch &sc) {
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
  d.key_index = sc.key_index;
  d.num_keys = (uint32_t)t->km->num_keys;
  d.valid = sc.valid;
  return d;
}

int set_seal(BSSL_AMD_DTLS_SET *t, const BSSL_AMD_DTLS_SET_RECORDS *sr, void *stream) {
  const BSSL_AMD_DTLS_RECORDS *r = &sr->records;
  const uint64_t n = r->num_records;
  if (n == 0) return 1;
  const KeyMaterial *km = t->km;
  if (!on_key_device(km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Scratch sc(s, n, sr->num_runs, t->ad_stride(), false);
  if (!sc.buf) return 0;
  BatchDesc d = batch_desc(t, r, sc);
  DtlsSetPrepare p;
  fill_prepare(&p, t, sr, sc);
  p.rec.out_lengths = r->out_lengths;
  bool ok = hipMemsetAsync(sc.zeroed, 0, sc.zeroed_bytes, s) == hipSuccess;
  Timed prepare(s);
  if (t->dtls13) {
    // The fragment is content || type: the pre-pass of the TLS 1.3 padded seal
    // with no padding, as for one association (dtls_api.cc).
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
    ok = ok && launch_tls13_pad_seal(ps, stream) == 0;
    p.rec.lengths = sc.frag_len;
    d.in = r->out;
    d.lengths = sc.frag_len;
  } else {
    p.rec.types = r->types;
    p.rec.type = r->type;
  }
  ok = ok && launch_dtls_set_prepare(p, t->mask, stream) == 0;
  prepare.stop();
  ok = ok && launch_desc(km, d, false, stream) == 0;
  if (ok && t->dtls13) {
    Timed mask(s);
    const DtlsMaskSeal m = {n,           r->out,    r->offsets, sc.frag_len, r->record_stride,
                            r->record_len, r->prefix, r->suffix,  d.status,    nullptr};
    ok = launch_dtls_set_mask(m, t->slots, p.runs.num_slots, sc.key_index, t->mask, stream) == 0;
    mask.stop();
  }
  return finish(ok);
}

int set_open(BSSL_AMD_DTLS_SET *t, const BSSL_AMD_DTLS_SET_RECORDS *sr, void *stream) {
  const BSSL_AMD_DTLS_RECORDS *r = &sr->records;
  const uint64_t n = r->num_records;
  if (n == 0) return 1;
  const KeyMaterial *km = t->km;
  if (!on_key_device(km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Scratch sc(s, n, sr->num_runs, t->ad_stride(), true);
  if (!sc.buf) return 0;
  BatchDesc d = batch_desc(t, r, sc);
  uint8_t *types = r->types ? r->types : sc.types;
  DtlsSetPrepare p;
  fill_prepare(&p, t, sr, sc);
  p.rec.body = r->in;
  p.rec.types_out = t->dtls13 ? nullptr : r->types;
  p.rec.ad_lengths = sc.ad_len;
  p.rec.seqs = sc.seqs;
  bool ok = hipMemsetAsync(sc.zeroed, 0, sc.zeroed_bytes, s) == hipSuccess;
  Timed prepare(s);
  ok = ok && launch_dtls_set_prepare(p, t->mask, stream) == 0;
  prepare.stop();
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
    DtlsSetWindow w;
    memset(&w, 0, sizeof(w));
    w.w.n = n;
    w.w.out = r->out;
    w.w.offsets = r->offsets;
    w.w.lengths = r->lengths;
    w.w.record_stride = r->record_stride;
    w.w.record_len = r->record_len;
    w.w.status = d.status;
    w.w.out_lengths = r->out_lengths;
    w.w.set_lengths = !t->dtls13;
    w.w.types = t->dtls13 ? types : nullptr;
    w.w.seqs = sc.seqs;
    w.w.table = reinterpret_cast<uint64_t *>(sc.table);
    w.w.table_slots = sc.table_slots;
    w.slots = t->slots;
    w.num_runs = sr->num_runs;
    w.run_of = sc.run_of;
    w.run_won = sc.run_won;
    w.run_max = sc.run_max;
    w.old = sc.old;
    w.block_r = sc.block_r;
    w.block_s = sc.block_s;
    ok = launch_dtls_set_window(w, stream) == 0;
    window.stop();
  }
  return finish(ok);
}

// Columns of the slot array (copy_columns, set_api.h).
bool slot_columns(BSSL_AMD_DTLS_SET *t, size_t first, size_t n, size_t offset, size_t width,
                  void *host, bool to_host, void *stream) {
  return copy_columns(t->slots, sizeof(DtlsSetSlot), first, n, offset, width, host, to_host,
                      reinterpret_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

BSSL_AMD_DTLS_SET *BSSL_AMD_DTLS_SET_new(enum evp_aead_direction_t direction, uint16_t version,
                                         const EVP_AEAD *aead, size_t num_slots) {
  // The rules and codes of BSSL_AMD_DTLS_AEAD_new and the count rule of
  // BSSL_AMD_TLS_SET_new, all before any GPU call.
  const bool dtls13 = version == BSSL_AMD_DTLS1_3_VERSION;
  if ((!dtls13 && version != BSSL_AMD_DTLS1_2_VERSION) || !aead || num_slots == 0 ||
      num_slots > kMaxCount) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return nullptr;
  }
  if (aead->kind == kAeadAesCtrHmac || aead->kind == kAeadTlsCbc) {
    PUT_ERROR(CIPHER_R_CTRL_NOT_IMPLEMENTED);
    return nullptr;
  }
  const bool chacha = aead == EVP_aead_chacha20_poly1305();
  if (!chacha && aead != EVP_aead_aes_128_gcm() && aead != EVP_aead_aes_256_gcm()) {
    PUT_ERROR(CIPHER_R_UNSUPPORTED_KEY_SIZE);
    return nullptr;
  }
  BSSL_AMD_DTLS_SET *t = new (std::nothrow) bssl_amd_dtls_set_st;
  if (t)
    t->km = keyset_new(aead, num_slots, sizeof(DtlsSetSlot), reinterpret_cast<void **>(&t->slots));
  if (!t || !t->km) {
    delete t;
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  t->seal = direction == evp_aead_seal;
  t->dtls13 = dtls13;
  t->xor_nonce = dtls13 || chacha;
  t->mask = !dtls13 ? kDtlsMaskNone
            : chacha ? kDtlsMaskChaCha
                     : aead->key_len == 16 ? kDtlsMaskAes128 : kDtlsMaskAes256;
  return t;
}

void BSSL_AMD_DTLS_SET_free(BSSL_AMD_DTLS_SET *s) {
  if (!s) return;
  keyset_free(s->km, s->slots, sizeof(DtlsSetSlot));
  delete s;
}

size_t BSSL_AMD_DTLS_SET_num_slots(const BSSL_AMD_DTLS_SET *s) { return s ? s->km->num_keys : 0; }

size_t BSSL_AMD_DTLS_SET_prefix_len(const BSSL_AMD_DTLS_SET *s) { return s->prefix_len(); }

int BSSL_AMD_DTLS_SET_set_slots(BSSL_AMD_DTLS_SET *s, size_t first, size_t n, const uint8_t *keys,
                                const uint8_t *fixed_ivs, const uint8_t *sn_keys,
                                const uint16_t *epochs, const uint64_t *seqs, void *hip_stream) {
  // All checks before any GPU call.
  if (!range_ok(s, first, n)) return 0;
  if (n == 0) return 1;
  bool args = keys && fixed_ivs && epochs && (s->dtls13 ? sn_keys != nullptr : sn_keys == nullptr);
  for (size_t i = 0; args && i < n; i++)
    args = !(s->dtls13 && epochs[i] == 0) && !(seqs && seqs[i] > kDtlsMaxSequence);
  if (!args) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  KeyMaterial *km = s->km;
  if (!on_key_device(km)) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t key_len = km->aead->key_len;
  const size_t iv_len = s->xor_nonce ? 12 : 4;
  // The slots staged in host memory, wiped on every path once the copy has
  // read them.
  std::vector<DtlsSetSlot> host_slots(n);
  Wiped wipe{host_slots.data(), n * sizeof(DtlsSetSlot)};
  bool ok = true;
  for (size_t i = 0; i < n && ok; i++) {
    DtlsSetSlot &c = host_slots[i];
    memset(&c, 0, sizeof(c));  // an empty window at 0
    c.seq = s->seal && seqs ? seqs[i] : 0;
    pack_iv(fixed_ivs + i * iv_len, iv_len, &c.iv_lo, &c.iv_hi);
    c.epoch = epochs[i];
    c.live = 1;
    // The record-number key, expanded once as for one association.
    ok = mask_key_words(s->mask, sn_keys ? sn_keys + i * key_len : nullptr, key_len, c.sn);
  }
  return finish(ok && install_slots(km, s->slots, sizeof(DtlsSetSlot), first, n, keys,
                                    host_slots.data(), st));
}

int BSSL_AMD_DTLS_SET_clear_slots(BSSL_AMD_DTLS_SET *s, size_t first, size_t n, void *hip_stream) {
  if (!range_ok(s, first, n)) return 0;
  if (n == 0) return 1;
  if (!on_key_device(s->km)) return 0;
  return finish(clear_slots(s->km, s->slots, sizeof(DtlsSetSlot), first, n,
                            reinterpret_cast<hipStream_t>(hip_stream)));
}

int BSSL_AMD_DTLS_SET_sequences(BSSL_AMD_DTLS_SET *s, size_t first, size_t n, uint64_t *out,
                                void *hip_stream) {
  if (!range_ok(s, first, n) || !direction_ok(s->seal, true)) return 0;
  if (n == 0) return 1;
  if (!present(out) || !on_key_device(s->km)) return 0;
  return finish(slot_columns(s, first, n, offsetof(DtlsSetSlot, seq), 8, out, true, hip_stream));
}

int BSSL_AMD_DTLS_SET_get_windows(BSSL_AMD_DTLS_SET *s, size_t first, size_t n, uint64_t *max_seqs,
                                  uint8_t *bitmaps, void *hip_stream) {
  if (!range_ok(s, first, n) || !direction_ok(s->seal, false)) return 0;
  if (n == 0) return 1;
  if (!present(max_seqs) || !present(bitmaps) || !on_key_device(s->km)) return 0;
  // max_seq and the map lie together in a slot (little-endian host: bit k of
  // the map is byte k / 8, bit k % 8).
  std::vector<uint64_t> w(5 * n);
  const bool ok =
      slot_columns(s, first, n, offsetof(DtlsSetSlot, max_seq), 40, w.data(), true, hip_stream);
  for (size_t i = 0; i < n; i++) {
    max_seqs[i] = ok ? w[5 * i] : 0;
    if (ok)
      memcpy(bitmaps + 32 * i, &w[5 * i + 1], 32);
    else
      memset(bitmaps + 32 * i, 0, 32);
  }
  return finish(ok);
}

int BSSL_AMD_DTLS_SET_set_windows(BSSL_AMD_DTLS_SET *s, size_t first, size_t n,
                                  const uint64_t *max_seqs, const uint8_t *bitmaps,
                                  void *hip_stream) {
  if (!range_ok(s, first, n) || !direction_ok(s->seal, false)) return 0;
  if (n == 0) return 1;
  if (!present(max_seqs) || !present(bitmaps)) return 0;
  for (size_t i = 0; i < n; i++)
    if (max_seqs[i] > kDtlsMaxSequence) {
      PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
      return 0;
    }
  if (!on_key_device(s->km)) return 0;
  std::vector<uint64_t> w(5 * n);
  for (size_t i = 0; i < n; i++) {
    w[5 * i] = max_seqs[i];
    memcpy(&w[5 * i + 1], bitmaps + 32 * i, 32);
  }
  return finish(
      slot_columns(s, first, n, offsetof(DtlsSetSlot, max_seq), 40, w.data(), false, hip_stream));
}

int BSSL_AMD_DTLS_SET_seal_records_device(BSSL_AMD_DTLS_SET *s, const BSSL_AMD_DTLS_SET_RECORDS *r,
                                          void *hip_stream) {
  return set_args_ok(s, r, true) ? set_seal(s, r, hip_stream) : 0;
}

int BSSL_AMD_DTLS_SET_open_records_device(BSSL_AMD_DTLS_SET *s, const BSSL_AMD_DTLS_SET_RECORDS *r,
                                          void *hip_stream) {
  return set_args_ok(s, r, false) ? set_open(s, r, hip_stream) : 0;
}

}  // extern "C"
