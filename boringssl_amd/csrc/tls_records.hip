// tls_records.hip -- per-record inputs of the TLS record layer, built on the
// device for a batch of records of one connection direction.
//
// Reference (one record per call): do_seal_record (ssl/tls_record.cc:266-317)
// writes the 5-byte header (TLS 1.3: outer type application_data, the real
// type sealed as `extra_in`), then SSLAEADContext::SealScatter
// (ssl/ssl_aead_ctx.cc:299-380) forms the nonce -- TLS 1.2 AES-GCM: 4-byte
// fixed IV || be64(seq), the 8 explicit bytes also written after the header;
// TLS 1.3 and TLS 1.2 ChaCha20-Poly1305: fixed_iv XOR (0^4 || be64(seq)) --
// and the additional data (GetAdditionalData, :207-224): TLS 1.2
// be64(seq) || type || version || be16(plaintext length), TLS 1.3 the header.
// The TLS 1.1 / 1.2 CBC suites (ssl_aead_ctx.cc:95-114) have a kernel of their
// own, tls_cbc_prepare_kernel: a 16-byte explicit IV -- the reference's
// RAND_bytes per record, here a ChaCha20 block per sequence number -- an AD
// without the length, and the header with the padded length.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "chacha_block.h"
#include "tls_prepare.h"

namespace bssl_amd {
namespace {

// The per-record body is tls_prepare_record (tls_prepare.h), shared with the
// connection sets' prepare kernel (tls_set.hip).
__global__ void tls_prepare_kernel(TlsPrepare p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  tls_prepare_record(p, i, p.seq + i, TlsIv::from_bytes(p.fixed_iv));
}

// Bytes 0..15 of the ChaCha20 block (RFC 8439 2.3) of `key` with block counter
// (uint32)seq and nonce words (uint32)(seq >> 32), 0, 0: one block per
// sequence number.  The first 16 bytes are words 0..3, little-endian.
__device__ void chacha_iv(const uint32_t (&key)[8], uint64_t seq, uint8_t *iv) {
  uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
  for (int k = 0; k < 8; k++) in[4 + k] = key[k];
  in[12] = (uint32_t)seq;
  in[13] = (uint32_t)(seq >> 32);
  in[14] = 0;
  in[15] = 0;
  uint32_t head[4];
  chacha20_block_head(in, head);
  for (int k = 0; k < 4; k++)
    for (int j = 0; j < 4; j++) iv[4 * k + j] = (uint8_t)(head[k] >> (8 * j));
}

// The CBC suites (TLS 1.1 / 1.2, explicit IV): SSLAEADContext::SealScatter /
// ::Open with random_variable_nonce_ and omit_length_in_ad_
// (ssl_aead_ctx.cc:109-113), do_seal_record's header and tls_open_record's
// public checks (tls_record.cc:117-133).
__global__ void tls_cbc_prepare_kernel(TlsCbcPrepare p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const uint64_t len = p.lengths ? p.lengths[i] : p.record_len;
  const uint64_t seq = p.seq + i;
  uint8_t *pre = p.prefix + 21 * i;
  uint8_t *nonce = p.nonces + 16 * i;
  uint8_t type;
  if (p.open) {
    type = pre[0];
    const uint32_t version = ((uint32_t)pre[1] << 8) | pre[2];
    const uint64_t hlen = ((uint64_t)pre[3] << 8) | pre[4];
    for (int k = 0; k < 16; k++) nonce[k] = pre[5 + k];
    if (p.types_out) p.types_out[i] = type;
    // The version, the length the header states, SSL3_RT_MAX_ENCRYPTED_LENGTH,
    // and what e_tls.cc:315-319 rejects before it decrypts.
    if (version != p.record_version || len > kTlsMaxEncryptedLen - 16 || hlen != 16 + len ||
        (len & 15) != 0 || len < p.mac_len + 1)
      p.valid[i] = 0;
  } else {
    type = p.types ? p.types[i] : p.type;
    if (p.explicit_ivs) {
      for (int k = 0; k < 16; k++) nonce[k] = p.explicit_ivs[16 * i + k];
    } else {
      chacha_iv(p.iv_key, seq, nonce);
    }
    // The fragment: IV, plaintext, MAC and the minimal padding.
    const uint64_t ctlen = 16 + len + p.mac_len + (16 - (len + p.mac_len) % 16);
    pre[0] = type;
    pre[1] = (uint8_t)(p.record_version >> 8);
    pre[2] = (uint8_t)p.record_version;
    pre[3] = (uint8_t)(ctlen >> 8);
    pre[4] = (uint8_t)ctlen;
    for (int k = 0; k < 16; k++) pre[5 + k] = nonce[k];
    if (len > kTlsMaxPlainLen) p.valid[i] = 0;
  }
  // GetAdditionalData without the length (ssl_aead_ctx.cc:207-224).
  uint8_t *ad = p.ad + 11 * i;
  for (int k = 0; k < 8; k++) ad[k] = (uint8_t)(seq >> (8 * (7 - k)));
  ad[8] = type;
  ad[9] = (uint8_t)(p.record_version >> 8);
  ad[10] = (uint8_t)p.record_version;
}

}  // namespace

int launch_tls_cbc_prepare(const TlsCbcPrepare &p, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tls_cbc_prepare_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s,
                     p);
  return (int)hipGetLastError();
}

int launch_tls_prepare(const TlsPrepare &p, void *stream) {
  if (p.n == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tls_prepare_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
  return (int)hipGetLastError();
}

}  // namespace bssl_amd
