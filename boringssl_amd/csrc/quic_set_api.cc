// quic_set_api.cc -- the C ABI of BSSL_AMD_QUIC_SET (include/bssl_amd/tls.h):
// one direction of many QUIC connections over device batches of packets.
//
// What BSSL_AMD_QUIC_AEAD (quic_api.cc) is for one connection and
// BSSL_AMD_DTLS_SET (dtls_set_api.cc) for many DTLS associations, composed: a
// keyset plus one QuicSetSlot per slot on the device -- IV, header-protection
// key, the next packet number or `expected` -- so that a batch that mixes the
// packets of many connections is one call that only enqueues work: the claim /
// prepare / advance kernels of quic_set.hip, the bulk kernels of the AEAD with
// a key index per packet (launch_desc), then on seal the tag and the
// header-protection mask, on open the per-slot `expected` update.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <vector>

#include "bssl_amd/tls.h"
#include "api_internal.h"

using namespace bssl_amd;

struct bssl_amd_quic_set_st {
  KeyMaterial *km;     // the keyset: num_slots keys, zero until installed
  QuicSetSlot *slots;  // device, num_slots entries
  bool seal;
  int mask;            // DtlsMask
};

namespace {

constexpr uint32_t kTagLen = 16;
constexpr size_t kMaxCount = 0xfffffffeu;  // slots, runs and packets of a call

// The scratch of one call, one stream-ordered block freed in stream order on
// every path.  Per packet: the body's offset and length, the header length,
// the packet number (open), the tag, the key index, the run, the nonce, the
// flag and a status byte for a caller who passes none; per run: who won; the
// flag word (QuicSetPrepare).
struct SetScratch {
  hipStream_t s;
  uint8_t *buf = nullptr;
  uint64_t *body_off, *body_len, *ad_len, *pns, *zeroed;
  uint32_t *flag, *key_index, *run_of, *run_won;
  uint8_t *tags, *nonce, *valid, *status;
  SetScratch(hipStream_t stream, uint64_t n, uint64_t runs) : s(stream) {
    if (bssl_amd::scratch_alloc(reinterpret_cast<void **>(&buf),
                                n * (4 * 8 + 16 + 2 * 4 + 12 + 2) + 8 + 4 * runs, s) != hipSuccess) {
      buf = nullptr;
      PUT_ERROR(ERR_R_MALLOC_FAILURE);
      return;
    }
    body_off = reinterpret_cast<uint64_t *>(buf);
    body_len = body_off + n;
    ad_len = body_len + n;
    pns = ad_len + n;
    tags = reinterpret_cast<uint8_t *>(pns + n);  // (16-byte aligned: 32 n bytes in)
    zeroed = reinterpret_cast<uint64_t *>(tags + 16 * n);  // the flag word
    flag = reinterpret_cast<uint32_t *>(zeroed);
    key_index = reinterpret_cast<uint32_t *>(zeroed + 1);
    run_of = key_index + n;
    run_won = run_of + n;
    nonce = reinterpret_cast<uint8_t *>(run_won + runs);
    valid = nonce + 12 * n;
    status = valid + n;
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
bool range_ok(const BSSL_AMD_QUIC_SET *t, size_t first, size_t n) {
  if (t && first <= t->km->num_keys && n <= t->km->num_keys - first) return true;
  return fail(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
}

// A call that reads or writes what only the other direction keeps.
bool direction_ok(const BSSL_AMD_QUIC_SET *t, bool want_seal) {
  return t->seal == want_seal ? true : fail(CIPHER_R_INVALID_OPERATION);
}

// The checks both packet calls share; false with the error queued.
bool set_args_ok(const BSSL_AMD_QUIC_SET *t, const BSSL_AMD_QUIC_SET_PACKETS *sp, bool want_seal) {
  if (!present(t) || !direction_ok(t, want_seal)) return false;
  if (!sp) return fail(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
  const BSSL_AMD_QUIC_PACKETS *p = &sp->packets;
  if (p->num_packets == 0) return true;
  if (p->in && p->out &&
      !(want_seal && !p->pn_lengths && (p->pn_length < 1 || p->pn_length > 4)) &&
      sp->num_runs != 0 && sp->run_slot && sp->run_start && sp->num_runs <= kMaxCount &&
      p->num_packets <= kMaxCount)
    return true;
  return fail(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
}

void fill_prepare(QuicSetPrepare *k, const BSSL_AMD_QUIC_SET *t, const BSSL_AMD_QUIC_SET_PACKETS *sp,
                  const SetScratch &sc) {
  const BSSL_AMD_QUIC_PACKETS *p = &sp->packets;
  memset(k, 0, sizeof(*k));
  k->pk.n = p->num_packets;
  k->pk.in = p->in;
  k->pk.out = p->out;
  k->pk.offsets = p->offsets;
  k->pk.lengths = p->lengths;
  k->pk.packet_stride = p->packet_stride;
  k->pk.packet_len = p->packet_len;
  k->pk.pn_offsets = p->pn_offsets;
  k->pk.pn_offset = p->pn_offset;
  k->pk.open = !t->seal;
  k->pk.nonces = sc.nonce;
  k->pk.valid = sc.valid;
  k->pk.tags = sc.tags;
  k->pk.body_offsets = sc.body_off;
  k->pk.body_lengths = sc.body_len;
  k->pk.ad_lengths = sc.ad_len;
  k->pk.pns = sc.pns;
  k->pk.packet_numbers = p->packet_numbers;
  k->slots = t->slots;
  k->num_slots = (uint32_t)t->km->num_keys;
  k->num_runs = sp->num_runs;
  k->run_slot = sp->run_slot;
  k->run_start = sp->run_start;
  k->key_index = sc.key_index;
  k->flag = sc.flag;
  k->run_of = sc.run_of;
  k->run_won = sc.run_won;
}

// The packets as the bulk kernels see them: record i is the body, its AD the
// header that the prepare step left in `out`, its tag in the scratch, its key
// the slot's.  Always the ragged description: a set needs `valid` for the
// packets that have no slot, so the uniform-shape ChaCha20 seal shortcut of
// quic_api.cc (which drops it) does not apply.
BatchDesc batch_desc(const BSSL_AMD_QUIC_SET *t, const BSSL_AMD_QUIC_PACKETS *p,
                     const SetScratch &sc) {
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
  d.key_index = sc.key_index;
  d.num_keys = (uint32_t)t->km->num_keys;
  d.valid = sc.valid;
  d.any_align = 1;  // a body starts where its header ends
  return d;
}

int set_seal(BSSL_AMD_QUIC_SET *t, const BSSL_AMD_QUIC_SET_PACKETS *sp, void *stream) {
  const BSSL_AMD_QUIC_PACKETS *p = &sp->packets;
  const uint64_t n = p->num_packets;
  if (n == 0) return 1;
  const KeyMaterial *km = t->km;
  if (!on_key_device(km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SetScratch sc(s, n, sp->num_runs);
  if (!sc.buf) return 0;
  const BatchDesc d = batch_desc(t, p, sc);
  QuicSetPrepare k;
  fill_prepare(&k, t, sp, sc);
  k.pk.pn_lengths = p->pn_lengths;
  k.pk.pn_length = p->pn_length;
  bool ok = hipMemsetAsync(sc.zeroed, 0, 8, s) == hipSuccess;
  Timed prepare(s);
  ok = ok && launch_quic_set_prepare(k, t->mask, stream) == 0;
  prepare.stop();
  ok = ok && launch_desc(km, d, false, stream) == 0;
  if (ok) {
    Timed protect(s);
    const QuicProtect m = {n,           p->out,      p->offsets, p->lengths, p->packet_stride,
                           p->packet_len, sc.body_off, sc.body_len, sc.tags,   d.status,
                           p->out_lengths, nullptr};
    ok = launch_quic_set_protect(m, t->slots, k.num_slots, sc.key_index, t->mask, stream) == 0;
    protect.stop();
  }
  return finish(ok);
}

int set_open(BSSL_AMD_QUIC_SET *t, const BSSL_AMD_QUIC_SET_PACKETS *sp, void *stream) {
  const BSSL_AMD_QUIC_PACKETS *p = &sp->packets;
  const uint64_t n = p->num_packets;
  if (n == 0) return 1;
  const KeyMaterial *km = t->km;
  if (!on_key_device(km)) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SetScratch sc(s, n, sp->num_runs);
  if (!sc.buf) return 0;
  const BatchDesc d = batch_desc(t, p, sc);
  QuicSetPrepare k;
  fill_prepare(&k, t, sp, sc);
  k.pk.header_lengths = p->header_lengths;
  bool ok = hipMemsetAsync(sc.zeroed, 0, 8, s) == hipSuccess;
  Timed prepare(s);
  ok = ok && launch_quic_set_prepare(k, t->mask, stream) == 0;
  prepare.stop();
  ok = ok && launch_desc(km, d, true, stream) == 0;
  if (ok) {
    Timed expected(s);
    const QuicSetExpected e = {{n, d.status, sc.pns, sc.body_len, p->out_lengths, nullptr},
                               t->slots, k.num_slots, sp->num_runs, sc.run_of, sc.run_won};
    ok = launch_quic_set_expected(e, stream) == 0;
    expected.stop();
  }
  return finish(ok);
}

// The slots' numbers to or from a packed host array; waits for the stream.
bool copy_numbers(BSSL_AMD_QUIC_SET *t, size_t first, size_t n, uint64_t *host, bool to_host,
                  hipStream_t s) {
  uint8_t *dev = reinterpret_cast<uint8_t *>(t->slots + first) + offsetof(QuicSetSlot, pn);
  const hipError_t e =
      to_host ? hipMemcpy2DAsync(host, 8, dev, sizeof(QuicSetSlot), 8, n, hipMemcpyDeviceToHost, s)
              : hipMemcpy2DAsync(dev, sizeof(QuicSetSlot), host, 8, 8, n, hipMemcpyHostToDevice, s);
  // (The copy reads or writes the caller's frame: wait until it has.)
  return hipStreamSynchronize(s) == hipSuccess && e == hipSuccess;
}

int get_numbers(BSSL_AMD_QUIC_SET *s, size_t first, size_t n, uint64_t *out, bool want_seal,
                void *hip_stream) {
  if (!range_ok(s, first, n) || !direction_ok(s, want_seal)) return 0;
  if (n == 0) return 1;
  if (!present(out) || !on_key_device(s->km)) return 0;
  return finish(copy_numbers(s, first, n, out, true, reinterpret_cast<hipStream_t>(hip_stream)));
}

}  // namespace

extern "C" {

BSSL_AMD_QUIC_SET *BSSL_AMD_QUIC_SET_new(enum evp_aead_direction_t direction, const EVP_AEAD *aead,
                                         size_t num_slots) {
  // The rules and codes of BSSL_AMD_QUIC_AEAD_new and the count rule of
  // BSSL_AMD_DTLS_SET_new, all before any GPU call.
  if (!aead || num_slots == 0 || num_slots > kMaxCount) {
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
  BSSL_AMD_QUIC_SET *t = new (std::nothrow) bssl_amd_quic_set_st;
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
  t->mask = chacha ? kDtlsMaskChaCha : aead->key_len == 16 ? kDtlsMaskAes128 : kDtlsMaskAes256;
  // All slots unset: zero keys, zero state.
  const size_t slot_bytes = num_slots * sizeof(QuicSetSlot);
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

void BSSL_AMD_QUIC_SET_free(BSSL_AMD_QUIC_SET *s) {
  if (!s) return;
  {
    DeviceGuard g(s->km->device);
    // As free_keys: drain the device, wipe, drain, free.
    hipDeviceSynchronize();
    hipMemset(s->slots, 0, s->km->num_keys * sizeof(QuicSetSlot));
    hipDeviceSynchronize();
    hipFree(s->slots);
  }
  free_keys(s->km);
  delete s;
}

size_t BSSL_AMD_QUIC_SET_num_slots(const BSSL_AMD_QUIC_SET *s) { return s ? s->km->num_keys : 0; }

int BSSL_AMD_QUIC_SET_set_slots(BSSL_AMD_QUIC_SET *s, size_t first, size_t n, const uint8_t *keys,
                                const uint8_t *ivs, const uint8_t *hp_keys,
                                const uint64_t *numbers, void *hip_stream) {
  // All checks before any GPU call.
  if (!range_ok(s, first, n)) return 0;
  if (n == 0) return 1;
  bool args = keys && ivs && hp_keys;
  // A sealing slot's first number is a packet number; `expected` may be 2^62.
  const uint64_t max_number = kQuicMaxPacketNumber + (s->seal ? 0 : 1);
  for (size_t i = 0; args && numbers && i < n; i++) args = numbers[i] <= max_number;
  if (!args) {
    PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
    return 0;
  }
  KeyMaterial *km = s->km;
  if (!on_key_device(km)) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t key_len = km->aead->key_len;
  const bool gcm = km->aead->kind == kAeadAesGcm;
  // The expanded keys and the slots staged in host memory, wiped on every path
  // once the copies have read them.
  std::vector<uint8_t> host_keys;
  std::vector<QuicSetSlot> host_slots(n);
  struct Wipe {
    std::vector<uint8_t> &k;
    std::vector<QuicSetSlot> &c;
    ~Wipe() {
      secure_zero(k.data(), k.size());
      secure_zero(c.data(), c.size() * sizeof(QuicSetSlot));
    }
  } wipe{host_keys, host_slots};
  bool ok = true;
  for (size_t i = 0; i < n && ok; i++) {
    QuicSetSlot &c = host_slots[i];
    memset(&c, 0, sizeof(c));
    c.pn = numbers ? numbers[i] : 0;
    const uint8_t *iv = ivs + 12 * i;
    for (int k = 0; k < 8; k++) c.iv_lo |= (uint64_t)iv[k] << (8 * k);
    for (int k = 8; k < 12; k++) c.iv_hi |= (uint32_t)iv[k] << (8 * (k - 8));
    c.live = 1;
    // The header-protection key, expanded once as for one connection.
    const uint8_t *hp = hp_keys + i * key_len;
    if (s->mask == kDtlsMaskChaCha) {
      for (int k = 0; k < 32; k++) c.hp[k / 4] |= (uint32_t)hp[k] << (8 * (k & 3));
    } else {
      CbcKeyDev ks;
      ok = cbc_key_setup(hp, key_len, &ks);
      memcpy(c.hp, ks.rk, sizeof(c.hp));
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
  ok = ok && hipMemcpyAsync(s->slots + first, host_slots.data(), n * sizeof(QuicSetSlot),
                            hipMemcpyHostToDevice, st) == hipSuccess;
  // The copies read pageable host memory that is wiped on return: wait until
  // they have.  (The host waits; the order on the stream is what the header
  // promises either way.)
  if (hipStreamSynchronize(st) != hipSuccess) ok = false;
  return finish(ok);
}

int BSSL_AMD_QUIC_SET_clear_slots(BSSL_AMD_QUIC_SET *s, size_t first, size_t n, void *hip_stream) {
  if (!range_ok(s, first, n)) return 0;
  if (n == 0) return 1;
  KeyMaterial *km = s->km;
  if (!on_key_device(km)) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const size_t per = km->aead->kind == kAeadAesGcm ? sizeof(GcmKeyDev) : sizeof(ChaChaKeyDev);
  return finish(
      hipMemsetAsync(static_cast<uint8_t *>(km->dev) + first * per, 0, n * per, st) == hipSuccess &&
      hipMemsetAsync(s->slots + first, 0, n * sizeof(QuicSetSlot), st) == hipSuccess);
}

int BSSL_AMD_QUIC_SET_next_packet_numbers(BSSL_AMD_QUIC_SET *s, size_t first, size_t n,
                                          uint64_t *out, void *hip_stream) {
  return get_numbers(s, first, n, out, true, hip_stream);
}

int BSSL_AMD_QUIC_SET_get_expected(BSSL_AMD_QUIC_SET *s, size_t first, size_t n, uint64_t *out,
                                   void *hip_stream) {
  return get_numbers(s, first, n, out, false, hip_stream);
}

int BSSL_AMD_QUIC_SET_set_expected(BSSL_AMD_QUIC_SET *s, size_t first, size_t n,
                                   const uint64_t *expected, void *hip_stream) {
  if (!range_ok(s, first, n) || !direction_ok(s, false)) return 0;
  if (n == 0) return 1;
  if (!present(expected)) return 0;
  for (size_t i = 0; i < n; i++)
    if (expected[i] > kQuicMaxPacketNumber + 1) {
      PUT_ERROR(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
      return 0;
    }
  if (!on_key_device(s->km)) return 0;
  return finish(copy_numbers(s, first, n, const_cast<uint64_t *>(expected), false,
                             reinterpret_cast<hipStream_t>(hip_stream)));
}

int BSSL_AMD_QUIC_SET_seal_packets_device(BSSL_AMD_QUIC_SET *s, const BSSL_AMD_QUIC_SET_PACKETS *p,
                                          void *hip_stream) {
  return set_args_ok(s, p, true) ? set_seal(s, p, hip_stream) : 0;
}

int BSSL_AMD_QUIC_SET_open_packets_device(BSSL_AMD_QUIC_SET *s, const BSSL_AMD_QUIC_SET_PACKETS *p,
                                          void *hip_stream) {
  return set_args_ok(s, p, false) ? set_open(s, p, hip_stream) : 0;
}

}  // extern "C"
