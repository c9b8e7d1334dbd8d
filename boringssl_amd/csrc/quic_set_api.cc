// quic_set_api.cc -- the C ABI of BSSL_AMD_QUIC_SET (include/bssl_amd/tls.h):
// one direction of many QUIC connections over device batches of packets.
//
// What BSSL_AMD_QUIC_AEAD (quic_api.cc) is for one connection and
// BSSL_AMD_DTLS_SET (dtls_set_api.cc) for many DTLS associations, composed: a
// keyset plus one QuicSetSlot per slot on the device -- IV, header-protection
// key, the next packet number or `expected` -- so that a batch that mixes the
// packets of many connections is one call that only enqueues work: the claim /
// prepare / advance launches of quic_set.hip, the bulk kernels of the AEAD with
// a key index per packet (launch_desc), then on seal the tag and the
// header-protection mask, on open the per-slot `expected` update.  The keyset,
// the slot array and the scratch block are set_api.h's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <vector>

#include "bssl_amd/tls.h"
#include "set_api.h"

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

using Scratch = CallScratch<QuicSetLayout>;

// The checks both packet calls share; false with the error queued.
bool set_args_ok(const BSSL_AMD_QUIC_SET *t, const BSSL_AMD_QUIC_SET_PACKETS *sp, bool want_seal) {
  if (!present(t) || !direction_ok(t->seal, want_seal)) return false;
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
                  const Scratch &sc) {
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
  k->runs = {(uint32_t)t->km->num_keys, sp->num_runs, sp->run_slot, sp->run_start,
             sc.key_index,              sc.flag,      sc.run_of,    sc.run_won};
}

// The packets as the bulk kernels see them: record i is the body, its AD the
// header that the prepare step left in `out`, its tag in the scratch, its key
// the slot's.  Always the ragged description: a set needs `valid` for the
// packets that have no slot, so the uniform-shape ChaCha20 seal shortcut of
// quic_api.cc (which drops it) does not apply.
BatchDesc batch_desc(const BSSL_AMD_QUIC_SET *t, const BSSL_AMD_QUIC_PACKETS *p,
                     const Scratch &sc) {
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
  Scratch sc(s, n, sp->num_runs);
  if (!sc.buf) return 0;
  const BatchDesc d = batch_desc(t, p, sc);
  QuicSetPrepare k;
  fill_prepare(&k, t, sp, sc);
  k.pk.pn_lengths = p->pn_lengths;
  k.pk.pn_length = p->pn_length;
  bool ok = hipMemsetAsync(sc.zeroed, 0, sc.zeroed_bytes, s) == hipSuccess;
  Timed prepare(s);
  ok = ok && launch_quic_set_prepare(k, t->mask, stream) == 0;
  prepare.stop();
  ok = ok && launch_desc(km, d, false, stream) == 0;
  if (ok) {
    Timed protect(s);
    const QuicProtect m = {n,           p->out,      p->offsets, p->lengths, p->packet_stride,
                           p->packet_len, sc.body_off, sc.body_len, sc.tags,   d.status,
                           p->out_lengths, nullptr};
    ok = launch_quic_set_protect(m, t->slots, k.runs.num_slots, sc.key_index, t->mask, stream) == 0;
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
  Scratch sc(s, n, sp->num_runs);
  if (!sc.buf) return 0;
  const BatchDesc d = batch_desc(t, p, sc);
  QuicSetPrepare k;
  fill_prepare(&k, t, sp, sc);
  k.pk.header_lengths = p->header_lengths;
  bool ok = hipMemsetAsync(sc.zeroed, 0, sc.zeroed_bytes, s) == hipSuccess;
  Timed prepare(s);
  ok = ok && launch_quic_set_prepare(k, t->mask, stream) == 0;
  prepare.stop();
  ok = ok && launch_desc(km, d, true, stream) == 0;
  if (ok) {
    Timed expected(s);
    const QuicSetExpected e = {{n, d.status, sc.pns, sc.body_len, p->out_lengths, nullptr},
                               t->slots, k.runs.num_slots, sp->num_runs, sc.run_of, sc.run_won};
    ok = launch_quic_set_expected(e, stream) == 0;
    expected.stop();
  }
  return finish(ok);
}

// The slots' numbers to or from a packed host array (copy_columns, set_api.h).
bool copy_numbers(BSSL_AMD_QUIC_SET *t, size_t first, size_t n, uint64_t *host, bool to_host,
                  hipStream_t s) {
  return copy_columns(t->slots, sizeof(QuicSetSlot), first, n, offsetof(QuicSetSlot, pn), 8, host,
                      to_host, s);
}

int get_numbers(BSSL_AMD_QUIC_SET *s, size_t first, size_t n, uint64_t *out, bool want_seal,
                void *hip_stream) {
  if (!range_ok(s, first, n) || !direction_ok(s->seal, want_seal)) return 0;
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
  BSSL_AMD_QUIC_SET *t = new (std::nothrow) bssl_amd_quic_set_st;
  if (t)
    t->km = keyset_new(aead, num_slots, sizeof(QuicSetSlot), reinterpret_cast<void **>(&t->slots));
  if (!t || !t->km) {
    delete t;
    PUT_ERROR(ERR_R_MALLOC_FAILURE);
    return nullptr;
  }
  t->seal = direction == evp_aead_seal;
  t->mask = chacha ? kDtlsMaskChaCha : aead->key_len == 16 ? kDtlsMaskAes128 : kDtlsMaskAes256;
  return t;
}

void BSSL_AMD_QUIC_SET_free(BSSL_AMD_QUIC_SET *s) {
  if (!s) return;
  keyset_free(s->km, s->slots, sizeof(QuicSetSlot));
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
  // The slots staged in host memory, wiped on every path once the copy has
  // read them.
  std::vector<QuicSetSlot> host_slots(n);
  Wiped wipe{host_slots.data(), n * sizeof(QuicSetSlot)};
  bool ok = true;
  for (size_t i = 0; i < n && ok; i++) {
    QuicSetSlot &c = host_slots[i];
    memset(&c, 0, sizeof(c));
    c.pn = numbers ? numbers[i] : 0;
    pack_iv(ivs + 12 * i, 12, &c.iv_lo, &c.iv_hi);
    c.live = 1;
    // The header-protection key, expanded once as for one connection.
    ok = mask_key_words(s->mask, hp_keys + i * key_len, key_len, c.hp);
  }
  return finish(ok && install_slots(km, s->slots, sizeof(QuicSetSlot), first, n, keys,
                                    host_slots.data(), st));
}

int BSSL_AMD_QUIC_SET_clear_slots(BSSL_AMD_QUIC_SET *s, size_t first, size_t n, void *hip_stream) {
  if (!range_ok(s, first, n)) return 0;
  if (n == 0) return 1;
  if (!on_key_device(s->km)) return 0;
  return finish(clear_slots(s->km, s->slots, sizeof(QuicSetSlot), first, n,
                            reinterpret_cast<hipStream_t>(hip_stream)));
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
  if (!range_ok(s, first, n) || !direction_ok(s->seal, false)) return 0;
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
