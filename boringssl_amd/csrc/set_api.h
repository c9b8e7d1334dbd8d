// set_api.h -- what the host sources of the three sets share (BSSL_AMD_TLS_SET
// in tls_api.cc, dtls_set_api.cc, quic_set_api.cc): a set is a keyset
// (KeyMaterial, one key per slot) plus an array of per-slot state on the
// device (TlsSetConn, DtlsSetSlot, QuicSetSlot), both all zero until a slot is
// installed.  Here: their allocation and wiped release, the install of keys
// and state, the clear, the strided copy of one field of the state, and the
// scratch block of a call.  Host only.
#ifndef BSSL_AMD_SET_API_H
#define BSSL_AMD_SET_API_H

#include "api_internal.h"
#include "set_scratch.h"

namespace bssl_amd {

// A zeroed keyset of num_slots keys of `aead` (AES-GCM or ChaCha20-Poly1305)
// and, in *slots, num_slots zeroed entries of slot_bytes on the current
// device.  Null when anything fails, with nothing left allocated; the caller
// queues the error.
KeyMaterial *keyset_new(const EVP_AEAD *aead, size_t num_slots, size_t slot_bytes, void **slots);
// Drains the device, wipes keys and state, drains, frees (as free_keys).
void keyset_free(KeyMaterial *km, void *slots, size_t slot_bytes);
// Slots first .. first + n - 1 get the keys (key_len bytes each) and the state
// the caller staged in host_slots (n entries of slot_bytes).  64 AES-GCM keys
// or more are expanded on the device (kDeviceKeySetupMin), fewer and ChaCha20's
// on the host, staged and wiped here on every path.  Waits for the stream: the
// copies read pageable host memory that the caller wipes on return.  (The host
// waits; the order on the stream is what the headers promise either way.)
bool install_slots(KeyMaterial *km, void *slots, size_t slot_bytes, size_t first, size_t n,
                   const uint8_t *keys, const void *host_slots, hipStream_t s);
// Zero keys, zero state, in stream order.
bool clear_slots(KeyMaterial *km, void *slots, size_t slot_bytes, size_t first, size_t n,
                 hipStream_t s);
// Columns of the slot array to or from a packed host array: `width` bytes at
// `offset` of each of slots first .. first + n - 1; waits for the stream (the
// copy reads or writes the caller's memory).
bool copy_columns(void *slots, size_t slot_bytes, size_t first, size_t n, size_t offset,
                  size_t width, void *host, bool to_host, hipStream_t s);
// A fixed IV of len <= 12 bytes, zero-extended, as the slots hold it: bytes
// 0..7 and 8..11, little-endian (TlsIv, tls_prepare.h).
void pack_iv(const uint8_t *bytes, size_t len, uint64_t *lo, uint32_t *hi);

// Wipes host memory that held secrets when the scope ends, on every path.
struct Wiped {
  void *p;
  size_t bytes;
  ~Wiped() { secure_zero(p, bytes); }
};

// The scratch of one call: one stream-ordered block laid out by Layout
// (set_scratch.h), freed in stream order on every path.  buf null: the
// allocation failed and the error is queued.
template <class Layout>
struct CallScratch : Layout {
  hipStream_t s;
  void *buf;
  template <class... A>
  explicit CallScratch(hipStream_t stream, A... a) : Layout(a...), s(stream) {
    size_t bytes;
    buf = carve_block(
        this,
        [&](size_t b) {
          void *p = nullptr;
          return scratch_alloc(&p, b, s) == hipSuccess ? p : nullptr;
        },
        &bytes);
    if (!buf) PUT_ERROR(ERR_R_MALLOC_FAILURE);
  }
  ~CallScratch() {
    if (buf) scratch_free(buf, s);
  }
  CallScratch(const CallScratch &) = delete;
  CallScratch &operator=(const CallScratch &) = delete;
};

}  // namespace bssl_amd

#endif
