// dtls_set_api.cc -- the C ABI of BSSL_AMD_DTLS_SET (include/bssl_amd/tls.h):
// one direction of many DTLS 1.2 / 1.3 associations over device batches.
//
// What BSSL_AMD_DTLS_AEAD (dtls_api.cc) is for one association and
// BSSL_AMD_TLS_SET (tls_api.cc) for many TLS connections, composed: a keyset
// plus one DtlsSetSlot per slot on the device -- fixed IV, epoch, record-number
// key, write sequence number, replay window -- so that a batch that mixes the
// records of many associations is one call that only enqueues work: the
// claim / prepare / advance kernels of dtls_set.hip, the bulk kernels of the
// AEAD with a key index per record (launch_desc), then on seal the DTLS 1.3
// record-number mask, on open the DTLS 1.3 strip (tls_pad.hip) and the
// per-slot replay windows.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <vector>

#include "bssl_amd/tls.h"
#include "api_internal.h"

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

// The scratch of one call, one stream-ordered block freed in stream order on
// every path.  Per record: the fragment length (DTLS 1.3 seal), the sequence
// number and the AD length (open), the key index, the run, the nonce, the AD,
// the flag, a status byte and a type byte for a caller who passes none; per
// run: who won, and for an open the run's maximum and its slot's old window;
// the flag word; for an open the index table and the workgroup maxima
// (DtlsSetPrepare, DtlsSetWindow).
struct SetScratch {
  hipStream_t s;
  uint8_t *buf = nullptr;
  uint64_t *frag_len, *seqs, *ad_len, *zeroed, *run_max, *old, *block_s;
  uint32_t *flag, *key_index, *run_of, *run_won, *block_r, *table;
  uint64_t table_slots = 0, zeroed_bytes;
  uint8_t *nonce, *ad, *valid, *status, *types;
  SetScratch(hipStream_t stream, uint64_t n, uint64_t runs, uint32_t ad_stride, bool open)
      : s(stream) {
    const uint64_t nb = open ? (n + 255) / 256 : 0, wruns = open ? runs : 0;
    if (open)
      for (table_slots = 512; table_slots < 2 * n;) table_slots *= 2;
    const uint64_t words8 = 3 * n + 1 + 7 * wruns + nb;
    const uint64_t words4 = 2 * n + runs + nb + table_slots;
    if (bssl_amd::scratch_alloc(reinterpret_cast<void **>(&buf),
                       8 * words8 + 4 * words4 + n * (12 + ad_stride + 3), s) != hipSuccess) {
      buf = nullptr;
      PUT_ERROR(ERR_R_MALLOC_FAILURE);
      return;
    }
    frag_len = reinterpret_cast<uint64_t *>(buf);
    seqs = frag_len + n;
    ad_len = seqs + n;
    zeroed = ad_len + n;  // the flag word, then the runs' maxima
    flag = reinterpret_cast<uint32_t *>(zeroed);
    run_max = zeroed + 1;
    zeroed_bytes = 8 * (1 + wruns);
    old = run_max + wruns;
    block_s = old + 6 * wruns;
    key_index = reinterpret_cast<uint32_t *>(block_s + nb);
    run_of = key_index + n;
    run_won = run_of + n;
    block_r = run_won + runs;
    table = block_r + nb;
    nonce = reinterpret_cast<uint8_t *>(table + table_slots);
    ad = nonce + 12 * n;
    valid = ad + ad_stride * n;
    status = valid + n;
    types = status + n;
  }
  ~SetScratch() {
    if (buf) bssl_amd::scratch_free(buf, s);
  }
  SetScratch(const SetScratch &) = delete;
  SetScratch &operator=(const SetScratch &) = delete;
};

bool fail(int reason) {
  PUT_ERROR(reason);
  return false;
}

bool present(const void *p) { return p ? true : fail(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED); }

int finish(bool ok) {
  if (ok) return 1;
  PUT_ERROR(ERR_R_INTERNAL_ERROR);
  return 0;
}

// Whether slots first .. first + n - 1 are inside the set.
bool range_ok(const BSSL_AMD_DTLS_SET *t, size_t first, size_t n) {
  if (t && first <= t->km->num_keys && n <= t->km->num_keys - first) return true;
  return fail(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
}

// A call that reads or writes what only the other direction keeps.
bool direction_ok(const BSSL_AMD_DTLS_SET *t, bool want_seal) {
  return t->seal == want_seal ? true : fail(CIPHER_R_INVALID_OPERATION);
}

// The checks both record calls share; false with the error queued.
bool set_args_ok(const BSSL_AMD_DTLS_SET *t, const BSSL_AMD_DTLS_SET_RECORDS *sr, bool want_seal) {
  if (!present(t) || !direction_ok(t, want_seal)) return false;
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
                  const SetScratch &sc) {
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
  p->num_slots = (uint32_t)t->km->num_keys;
  p->num_runs = sr->num_runs;
  p->run_slot = sr->run_slot;
  p->run_start = sr->run_start;
  p->key_index = sc.key_index;
  p->flag = sc.flag;
  p->run_of = sc.run_of;
  p->run_won = sc.run_won;
}

BatchDesc batch_desc(const BSSL_AMD_DTLS_SET *t, const BSSL_AMD_DTLS_RECORDS *r,
                     const SetScratch &sc) {
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
  SetScratch sc(s, n, sr->num_runs, t->ad_stride(), false);
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
    ok = launch_dtls_set_mask(m, t->slots, p.num_slots, sc.key_index, t->mask, stream) == 0;
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
  SetScratch sc(s, n, sr->num_runs, t->ad_stride(), true);
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

// Columns of the slot array to or from a packed host array: `width` bytes at
// `offset` of each of slots first .. first + n - 1; waits for the stream.
bool copy_columns(BSSL_AMD_DTLS_SET *t, size_t first, size_t n, size_t offset, size_t width,
                  void *host, bool to_host, hipStream_t s) {
  uint8_t *dev = reinterpret_cast<uint8_t *>(t->slots + first) + offset;
  const hipError_t e =
      to_host ? hipMemcpy2DAsync(host, width, dev, sizeof(DtlsSetSlot), width, n,
                                 hipMemcpyDeviceToHost, s)
              : hipMemcpy2DAsync(dev, sizeof(DtlsSetSlot), host, width, width, n,
                                 hipMemcpyHostToDevice, s);
  // (The copy reads or writes the caller's frame: wait until it has.)
  return hipStreamSynchronize(s) == hipSuccess && e == hipSuccess;
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
  int dev = 0;
  BSSL_AMD_DTLS_SET *t = new (std::nothrow) bssl_amd_dtls_set_st;
  KeyMaterial *km = t ? new (std::nothrow) KeyMaterial{aead, 0, num_slots, 0, nullptr, 0} : nullptr;
  if (!km || hipGetDevice(&dev) != hipSuccess) {
    delete km;
    delete t;
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  km->device = dev;
  km->nr = chacha ? 0 : (int)aead->key_len / 4 + 6;
  km->bytes = num_slots * (chacha ? sizeof(ChaChaKeyDev) : sizeof(GcmKeyDev));
  t->km = km;
  t->slots = nullptr;
  t->seal = direction == evp_aead_seal;
  t->dtls13 = dtls13;
  t->xor_nonce = dtls13 || chacha;
  t->mask = !dtls13 ? kDtlsMaskNone
            : chacha ? kDtlsMaskChaCha
                     : aead->key_len == 16 ? kDtlsMaskAes128 : kDtlsMaskAes256;
  // All slots unset: zero keys, zero state.
  const size_t slot_bytes = num_slots * sizeof(DtlsSetSlot);
  bool ok = hipMalloc(&km->dev, km->bytes) == hipSuccess;
  if (!ok) km->dev = nullptr;
  ok = ok && hipMalloc(reinterpret_cast<void **>(&t->slots), slot_bytes) == hipSuccess;
  ok = ok && hipMemset(km->dev, 0, km->bytes) == hipSuccess &&
       hipMemset(t->slots, 0, slot_bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    if (t->slots) hipFree(t->slots);
    if (km->dev) hipFree(km->dev);
    delete km;
    delete t;
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  return t;
}

void BSSL_AMD_DTLS_SET_free(BSSL_AMD_DTLS_SET *s) {
  if (!s) return;
  {
    DeviceGuard g(s->km->device);
    // As free_keys: drain the device, wipe, drain, free.
    hipDeviceSynchronize();
    hipMemset(s->slots, 0, s->km->num_keys * sizeof(DtlsSetSlot));
    hipDeviceSynchronize();
    hipFree(s->slots);
  }
  free_keys(s->km);
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
  const bool gcm = km->aead->kind == kAeadAesGcm;
  // The expanded keys and the slots staged in host memory, wiped on every path
  // once the copies have read them.
  std::vector<uint8_t> host_keys;
  std::vector<DtlsSetSlot> host_slots(n);
  struct Wipe {
    std::vector<uint8_t> &k;
    std::vector<DtlsSetSlot> &c;
    ~Wipe() {
      secure_zero(k.data(), k.size());
      secure_zero(c.data(), c.size() * sizeof(DtlsSetSlot));
    }
  } wipe{host_keys, host_slots};
  bool ok = true;
  for (size_t i = 0; i < n && ok; i++) {
    DtlsSetSlot &c = host_slots[i];
    memset(&c, 0, sizeof(c));  // an empty window at 0
    c.seq = s->seal && seqs ? seqs[i] : 0;
    uint8_t iv[12] = {0};
    memcpy(iv, fixed_ivs + i * iv_len, iv_len);
    for (int k = 0; k < 8; k++) c.iv_lo |= (uint64_t)iv[k] << (8 * k);
    for (int k = 8; k < 12; k++) c.iv_hi |= (uint32_t)iv[k] << (8 * (k - 8));
    secure_zero(iv, sizeof(iv));
    c.epoch = epochs[i];
    c.live = 1;
    // The record-number key, expanded once as for one association.
    const uint8_t *sn = sn_keys ? sn_keys + i * key_len : nullptr;
    if (s->mask == kDtlsMaskChaCha) {
      for (int k = 0; k < 32; k++) c.sn[k / 4] |= (uint32_t)sn[k] << (8 * (k & 3));
    } else if (s->mask != kDtlsMaskNone) {
      CbcKeyDev ks;
      ok = cbc_key_setup(sn, key_len, &ks);
      memcpy(c.sn, ks.rk, sizeof(c.sn));
      secure_zero(&ks, sizeof(ks));
    }
  }
  if (ok && gcm && n >= kDeviceKeySetupMin) {
    // The device key setup writes the tables straight into the slots (and
    // waits for the stream).
    ok = gcm_key_setup_device(keys, key_len, n, static_cast<GcmKeyDev *>(km->dev) + first, st) == 0;
  } else if (ok) {
    const size_t per = gcm ? sizeof(GcmKeyDev) : sizeof(ChaChaKeyDev);
    host_keys.resize(n * per);
    for (size_t i = 0; i < n && ok; i++) {
      if (gcm)
        ok = gcm_key_setup(keys + i * key_len, key_len,
                           reinterpret_cast<GcmKeyDev *>(host_keys.data()) + i);
      else
        chacha_key_setup(keys + i * key_len, reinterpret_cast<ChaChaKeyDev *>(host_keys.data()) + i);
    }
    ok = ok && hipMemcpyAsync(static_cast<uint8_t *>(km->dev) + first * per, host_keys.data(),
                              n * per, hipMemcpyHostToDevice, st) == hipSuccess;
  }
  ok = ok && hipMemcpyAsync(s->slots + first, host_slots.data(), n * sizeof(DtlsSetSlot),
                            hipMemcpyHostToDevice, st) == hipSuccess;
  // The copies read pageable host memory that is wiped on return: wait until
  // they have.  (The host waits; the order on the stream is what the header
  // promises either way.)
  if (hipStreamSynchronize(st) != hipSuccess) ok = false;
  return finish(ok);
}

int BSSL_AMD_DTLS_SET_clear_slots(BSSL_AMD_DTLS_SET *s, size_t first, size_t n, void *hip_stream) {
  if (!range_ok(s, first, n)) return 0;
  if (n == 0) return 1;
  KeyMaterial *km = s->km;
  if (!on_key_device(km)) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t per = km->aead->kind == kAeadAesGcm ? sizeof(GcmKeyDev) : sizeof(ChaChaKeyDev);
  return finish(
      hipMemsetAsync(static_cast<uint8_t *>(km->dev) + first * per, 0, n * per, st) == hipSuccess &&
      hipMemsetAsync(s->slots + first, 0, n * sizeof(DtlsSetSlot), st) == hipSuccess);
}

int BSSL_AMD_DTLS_SET_sequences(BSSL_AMD_DTLS_SET *s, size_t first, size_t n, uint64_t *out,
                                void *hip_stream) {
  if (!range_ok(s, first, n) || !direction_ok(s, true)) return 0;
  if (n == 0) return 1;
  if (!present(out) || !on_key_device(s->km)) return 0;
  return finish(copy_columns(s, first, n, offsetof(DtlsSetSlot, seq), 8, out, true,
                             reinterpret_cast<hipStream_t>(hip_stream)));
}

int BSSL_AMD_DTLS_SET_get_windows(BSSL_AMD_DTLS_SET *s, size_t first, size_t n, uint64_t *max_seqs,
                                  uint8_t *bitmaps, void *hip_stream) {
  if (!range_ok(s, first, n) || !direction_ok(s, false)) return 0;
  if (n == 0) return 1;
  if (!present(max_seqs) || !present(bitmaps) || !on_key_device(s->km)) return 0;
  // max_seq and the map lie together in a slot (little-endian host: bit k of
  // the map is byte k / 8, bit k % 8).
  std::vector<uint64_t> w(5 * n);
  const bool ok = copy_columns(s, first, n, offsetof(DtlsSetSlot, max_seq), 40, w.data(), true,
                               reinterpret_cast<hipStream_t>(hip_stream));
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
  if (!range_ok(s, first, n) || !direction_ok(s, false)) return 0;
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
  return finish(copy_columns(s, first, n, offsetof(DtlsSetSlot, max_seq), 40, w.data(), false,
                             reinterpret_cast<hipStream_t>(hip_stream)));
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
