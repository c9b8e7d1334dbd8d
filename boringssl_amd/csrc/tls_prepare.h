// tls_prepare.h -- the per-record body of the TLS record layer's prepare
// kernels, shared by tls_prepare_kernel (tls_records.hip: one connection, the
// sequence numbers seq .. seq + n - 1) and tls_set_prepare_kernel
// (tls_set.hip: many connections, every record its connection's IV and next
// sequence number).  One __device__ function, inlined into both (DESIGN.md
// 4.11a: one body, the differences in what the caller passes).
#ifndef BSSL_AMD_TLS_PREPARE_H
#define BSSL_AMD_TLS_PREPARE_H

#include "internal.h"

namespace bssl_amd {

// A connection's fixed IV by value (TLS 1.2 AES-GCM: 4 bytes, then zeros):
// bytes 0..7 in lo and 8..11 in hi, little-endian -- two scalars and no array,
// so that it stays in registers whatever the compiler unrolls.
struct TlsIv {
  uint64_t lo;
  uint32_t hi;
  __host__ __device__ uint8_t byte(int k) const {
    return k < 8 ? (uint8_t)(lo >> (8 * k)) : (uint8_t)(hi >> (8 * (k - 8)));
  }
  __host__ __device__ static TlsIv from_bytes(const uint8_t *b) {
    TlsIv iv = {0, 0};
    for (int k = 0; k < 8; k++) iv.lo |= (uint64_t)b[k] << (8 * k);
    for (int k = 8; k < 12; k++) iv.hi |= (uint32_t)b[k] << (8 * (k - 8));
    return iv;
  }
};

// Record i with sequence number seq and fixed IV iv: the nonce, on seal the
// header and explicit nonce into the prefix, the additional data, the TLS 1.3
// inner type, and valid[i] = 0 for a plaintext over 2^14 bytes (valid[i] is
// not written otherwise).  p.fixed_iv and p.seq are not read.
// The TLS 1.3 padded form (p.padded; tls_pad.hip) differs in what the caller
// passes -- lengths[i] is the fragment length F and there is no extra byte, so
// the header says F + 16 -- and in the flag: on seal it is the pre-pass's, on
// open it takes tls_open_record's checks of the received header.
__device__ __forceinline__ void tls_prepare_record(const TlsPrepare &p, uint64_t i, uint64_t seq,
                                                   const TlsIv &iv) {
  const uint64_t len = p.lengths ? p.lengths[i] : p.record_len;
  uint8_t *pre = p.prefix + p.prefix_len * i;
  // Seal: the caller's type; open: the received header's (tls_record.cc:197-235).
  // (p.type by value through readfirstlane -- it is uniform, so the value is
  // unchanged: otherwise the compiler turns the choice into a load through a
  // select between &p.types[i] and &p.type, which takes the address of a
  // kernel argument and costs a scratch slot.)
  uint8_t type = (uint8_t)__builtin_amdgcn_readfirstlane((uint32_t)p.type);
  if (p.open)
    type = pre[0];
  else if (p.types)
    type = p.types[i];
  // Nonce (ssl_aead_ctx.cc:326-365 seal, 248-279 open).
  uint8_t *nonce = p.nonces + 12 * i;
  for (int k = 0; k < 12; k++) {
    const uint8_t sb = k >= 4 ? (uint8_t)(seq >> (8 * (11 - k))) : 0;
    uint8_t v;
    if (p.xor_nonce)
      v = (uint8_t)(iv.byte(k) ^ sb);
    else if (k < 4)
      v = iv.byte(k);
    else
      v = p.open ? pre[5 + (k - 4)] : sb;  // the explicit nonce travels in the record
    nonce[k] = v;
  }
  // Header (seal): ciphertext length = explicit nonce + plaintext + extra + tag.
  uint8_t hdr[5];
  if (p.open) {
    for (int k = 0; k < 5; k++) hdr[k] = pre[k];
  } else {
    const uint64_t ctlen = p.explicit_len + len + p.extra_len + p.tag_len;
    hdr[0] = p.tls13 ? (uint8_t)23 : type;  // SSL3_RT_APPLICATION_DATA outside in TLS 1.3
    hdr[1] = (uint8_t)(p.record_version >> 8);
    hdr[2] = (uint8_t)p.record_version;
    hdr[3] = (uint8_t)(ctlen >> 8);
    hdr[4] = (uint8_t)ctlen;
    for (int k = 0; k < 5; k++) pre[k] = hdr[k];
    for (uint32_t k = 0; k < p.explicit_len; k++) pre[5 + k] = nonce[4 + k];
  }
  // Additional data (GetAdditionalData, ssl_aead_ctx.cc:207-224).
  uint8_t *ad = p.ad + p.ad_stride * i;
  if (p.tls13) {
    for (int k = 0; k < 5; k++) ad[k] = hdr[k];
  } else {
    for (int k = 0; k < 8; k++) ad[k] = (uint8_t)(seq >> (8 * (7 - k)));
    ad[8] = type;
    ad[9] = hdr[1];
    ad[10] = hdr[2];
    ad[11] = (uint8_t)(len >> 8);
    ad[12] = (uint8_t)len;
  }
  if (p.extra_len && !p.open) p.extra[i] = type;  // the inner content type (tls_record.cc:272-276)
  if (p.padded) {
    // Open: application_data outside (tls_record.cc:214), the record version
    // (:117-130), the stated length (which with the next bound is within
    // SSL3_RT_MAX_ENCRYPTED_LENGTH, :133), and a fragment of 1 .. 2^14 + 1
    // bytes (:204-209; an empty one has no type).
    const uint64_t hlen = ((uint64_t)hdr[3] << 8) | hdr[4];
    if (p.open && (hdr[0] != 23 || hdr[1] != (uint8_t)(p.record_version >> 8) ||
                   hdr[2] != (uint8_t)p.record_version || hlen != len + p.tag_len || len == 0 ||
                   len > kTlsMaxPlainLen + 1))
      p.valid[i] = 0;
    return;
  }
  // Plaintext records are at most 2^14 bytes (SSL3_RT_MAX_PLAIN_LENGTH); a
  // longer one fails like a rejected call.
  if (len > kTlsMaxPlainLen) p.valid[i] = 0;
}

}  // namespace bssl_amd

#endif
