// set_api.cc -- the slot-state helpers of set_api.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <vector>

#include "set_api.h"
#include "tls_prepare.h"

namespace bssl_amd {

namespace {

size_t key_bytes(const KeyMaterial *km) {
  return km->aead->kind == kAeadAesGcm ? sizeof(GcmKeyDev) : sizeof(ChaChaKeyDev);
}

}  // namespace

KeyMaterial *keyset_new(const EVP_AEAD *aead, size_t num_slots, size_t slot_bytes, void **slots) {
  *slots = nullptr;
  int dev = 0;
  KeyMaterial *km = new (std::nothrow) KeyMaterial{aead, 0, num_slots, 0, nullptr, 0};
  if (!km || hipGetDevice(&dev) != hipSuccess) {
    delete km;
    return nullptr;
  }
  km->device = dev;
  km->nr = aead->kind == kAeadAesGcm ? (int)aead->key_len / 4 + 6 : 0;
  km->bytes = num_slots * key_bytes(km);
  // All slots unset: zero keys, zero state.
  bool ok = hipMalloc(&km->dev, km->bytes) == hipSuccess;
  if (!ok) km->dev = nullptr;
  ok = ok && hipMalloc(slots, num_slots * slot_bytes) == hipSuccess;
  ok = ok && hipMemset(km->dev, 0, km->bytes) == hipSuccess &&
       hipMemset(*slots, 0, num_slots * slot_bytes) == hipSuccess &&
       hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    if (*slots) hipFree(*slots);
    if (km->dev) hipFree(km->dev);
    *slots = nullptr;
    delete km;
    return nullptr;
  }
  return km;
}

void keyset_free(KeyMaterial *km, void *slots, size_t slot_bytes) {
  {
    DeviceGuard g(km->device);
    hipDeviceSynchronize();
    hipMemset(slots, 0, km->num_keys * slot_bytes);
    hipDeviceSynchronize();
    hipFree(slots);
  }
  free_keys(km);
}

bool install_slots(KeyMaterial *km, void *slots, size_t slot_bytes, size_t first, size_t n,
                   const uint8_t *keys, const void *host_slots, hipStream_t s) {
  const size_t key_len = km->aead->key_len, per = key_bytes(km);
  const bool gcm = km->aead->kind == kAeadAesGcm;
  std::vector<uint8_t> host_keys;
  bool ok = true;
  if (gcm && n >= kDeviceKeySetupMin) {
    // The device key setup writes the tables straight into the slots (and
    // waits for the stream).
    ok = gcm_key_setup_device(keys, key_len, n, static_cast<GcmKeyDev *>(km->dev) + first, s) == 0;
  } else {
    host_keys.resize(n * per);
    for (size_t i = 0; i < n && ok; i++) {
      if (gcm)
        ok = gcm_key_setup(keys + i * key_len, key_len,
                           reinterpret_cast<GcmKeyDev *>(host_keys.data()) + i);
      else
        chacha_key_setup(keys + i * key_len, reinterpret_cast<ChaChaKeyDev *>(host_keys.data()) + i);
    }
    ok = ok && hipMemcpyAsync(static_cast<uint8_t *>(km->dev) + first * per, host_keys.data(),
                              n * per, hipMemcpyHostToDevice, s) == hipSuccess;
  }
  ok = ok && hipMemcpyAsync(static_cast<uint8_t *>(slots) + first * slot_bytes, host_slots,
                            n * slot_bytes, hipMemcpyHostToDevice, s) == hipSuccess;
  if (hipStreamSynchronize(s) != hipSuccess) ok = false;
  secure_zero(host_keys.data(), host_keys.size());
  return ok;
}

bool clear_slots(KeyMaterial *km, void *slots, size_t slot_bytes, size_t first, size_t n,
                 hipStream_t s) {
  const size_t per = key_bytes(km);
  return hipMemsetAsync(static_cast<uint8_t *>(km->dev) + first * per, 0, n * per, s) == hipSuccess &&
         hipMemsetAsync(static_cast<uint8_t *>(slots) + first * slot_bytes, 0, n * slot_bytes, s) ==
             hipSuccess;
}

bool copy_columns(void *slots, size_t slot_bytes, size_t first, size_t n, size_t offset,
                  size_t width, void *host, bool to_host, hipStream_t s) {
  uint8_t *dev = static_cast<uint8_t *>(slots) + first * slot_bytes + offset;
  const hipError_t e =
      to_host ? hipMemcpy2DAsync(host, width, dev, slot_bytes, width, n, hipMemcpyDeviceToHost, s)
              : hipMemcpy2DAsync(dev, slot_bytes, host, width, width, n, hipMemcpyHostToDevice, s);
  return hipStreamSynchronize(s) == hipSuccess && e == hipSuccess;
}

void pack_iv(const uint8_t *bytes, size_t len, uint64_t *lo, uint32_t *hi) {
  uint8_t iv[12] = {0};
  memcpy(iv, bytes, len);
  const TlsIv v = TlsIv::from_bytes(iv);
  *lo = v.lo;
  *hi = v.hi;
  secure_zero(iv, sizeof(iv));
}

}  // namespace bssl_amd
