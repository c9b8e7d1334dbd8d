// api_internal.h -- what the host C-ABI sources share: aead_api.cc defines it;
// the record and packet layers of bssl_amd/tls.h (tls_api.cc, dtls_api.cc,
// quic_api.cc and the sets, set_api.h) use it, with the argument and result
// helpers below.  Host only; the kernels see internal.h alone.
#ifndef BSSL_AMD_API_INTERNAL_H
#define BSSL_AMD_API_INTERNAL_H

#include "bssl_amd/aead.h"
#include "internal.h"

// AEAD method objects (the reference's struct evp_aead_st vtable,
// crypto/fipsmodule/cipher/internal.h:40-78, reduced to the parameters the
// GPU path needs).
struct evp_aead_st {
  uint8_t key_len;
  uint8_t nonce_len;
  uint8_t overhead;
  uint8_t max_tag_len;
  bssl_amd::AeadKind kind;
  int tls;  // 0, 12 or 13: the tls12 / tls13 monotonic-nonce variants
};

namespace bssl_amd {

// The thread's error queue (ERR_get_error), library ERR_LIB_CIPHER.
void put_error(int reason);
#define PUT_ERROR(reason) ::bssl_amd::put_error(reason)

// The argument and result helpers of the calls of bssl_amd/tls.h: each queues
// its error and returns false (finish: 0).
inline bool fail(int reason) {
  PUT_ERROR(reason);
  return false;
}
// A call without its context, set or a required array.
inline bool present(const void *p) { return p ? true : fail(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED); }
// A context or set of the other direction was called, or a call reads or
// writes what only the other direction keeps.
inline bool direction_ok(bool seal, bool want_seal) {
  return seal == want_seal ? true : fail(CIPHER_R_INVALID_OPERATION);
}
// The end of a call whose GPU work was enqueued (or not).
inline int finish(bool ok) { return ok ? 1 : (int)fail(ERR_R_INTERNAL_ERROR); }

// Device-resident key material for one or more keys.
struct KeyMaterial {
  const EVP_AEAD *aead;
  int device;  // the HIP device the key material lives on
  size_t num_keys;
  int nr;
  // GcmKeyDev[num_keys], CbcKeyDev[num_keys], AesHmacKeyDev[num_keys] or
  // ChaChaKeyDev[num_keys]
  void *dev;
  size_t bytes;
  // kAeadTlsCbc: the one direction the keys work in (e_tls.cc:125-129, 274-278).
  bool open_only = false;
};

// Whether slots first .. first + n - 1 are inside the set t (its keyset t->km).
template <class Set>
bool range_ok(const Set *t, size_t first, size_t n) {
  if (t && first <= t->km->num_keys && n <= t->km->num_keys - first) return true;
  return fail(ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED);
}

// Makes `dev` the calling thread's current HIP device for the guard's scope
// and restores the previous one (host-buffer calls may come from any thread,
// as the reference's EVP_AEAD_CTX allows, aead.h:298-299).
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) return;
    ok = prev == dev || hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (ok) hipSetDevice(prev);
  }
};

// State kept in EVP_AEAD_CTX.state (560 bytes, reference aead.h:222-235).
struct CtxState {
  KeyMaterial *km;
  uint64_t min_next_nonce;  // tls12/tls13 (e_aes.cc.inc:1041-1044, 1130-1134)
  uint64_t mask;
};
static_assert(sizeof(CtxState) <= sizeof(((EVP_AEAD_CTX *)nullptr)->state), "state");

inline CtxState *state_of(const EVP_AEAD_CTX *ctx) {
  return reinterpret_cast<CtxState *>(const_cast<uint8_t *>(ctx->state.opaque));
}

// Device-batch calls take device pointers and a stream of the caller's
// current device; they must be made on the device that holds the keys.
bool on_key_device(const KeyMaterial *km);
// Drains the device, wipes the device copy of the keys and frees it.
void free_keys(KeyMaterial *km);
// Launch the bulk kernels of the AEAD over a filled-in descriptor, with the
// timing pair and the kernel name of BSSL_AMD_set_kernel_timing.  Returns 0 or
// a HIP error code.  `gcm_eng`: the AES-GCM engine the caller already read for
// this batch (-1: read it here), so one batch never sees two engines.
int launch_desc(const KeyMaterial *km, const BatchDesc &d, bool open, void *stream,
                int gcm_eng = -1);
// With BSSL_AMD_set_kernel_timing on: a pair of events for a kernel that frames
// the bulk one (dtls_api.cc), reported by BSSL_AMD_collect_kernel_times in
// launch order with the bulk kernels' pairs; null otherwise.  The pointer holds
// until the next pair is taken.
const KernelEvents *kernel_timing_pair();
// Brackets the launches of one step of a call with such a pair (dtls_api.cc,
// the sets).
struct Timed {
  const KernelEvents *ev;
  hipStream_t s;
  explicit Timed(hipStream_t stream) : ev(kernel_timing_pair()), s(stream) {
    if (ev) hipEventRecord(reinterpret_cast<hipEvent_t>(ev->start), s);
  }
  // (Before the next pair is taken: the pointer holds until then.)
  void stop() {
    if (ev) hipEventRecord(reinterpret_cast<hipEvent_t>(ev->stop), s);
    ev = nullptr;
  }
};

// kAeadTlsCbc: the MAC size (e_tls.cc:105-116).
size_t tls_cbc_mac_len(const EVP_AEAD *aead);
uint64_t load_be64(const uint8_t *p);

}  // namespace bssl_amd

#endif
