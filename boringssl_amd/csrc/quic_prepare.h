// quic_prepare.h -- the per-packet body of QUIC packet protection (quic.hip:
// one direction of one key generation of one connection), one __device__
// function per step as dtls_prepare.h has for DTLS, so that kernels over many
// connections can share them: the differences are in what the caller passes
// (the packet number, the IV, `expected`, the header-protection key).
//
// RFC 9001 5.3 (the AEAD: nonce = iv XOR the packet number, AD = the header
// through the packet-number field), 5.4 (header protection: a 5-byte mask from
// a 16-byte sample taken 4 bytes after the start of the packet-number field),
// RFC 9000 17.1 and A.3 (the truncated packet number and its decoding).
#ifndef BSSL_AMD_QUIC_PREPARE_H
#define BSSL_AMD_QUIC_PREPARE_H

#include "dtls_prepare.h"

namespace bssl_amd {
namespace {

struct QuicPacket {
  uint64_t off, len;
  uint32_t pn_off;
};

__device__ __forceinline__ QuicPacket quic_packet(const uint64_t *offsets, const uint64_t *lengths,
                                                  uint64_t stride, uint64_t packet_len,
                                                  const uint32_t *pn_offsets, uint32_t pn_offset,
                                                  uint64_t i) {
  QuicPacket k;
  k.off = offsets ? offsets[i] : i * stride;
  k.len = lengths ? lengths[i] : packet_len;
  k.pn_off = pn_offsets ? pn_offsets[i] : pn_offset;
  return k;
}

// The five mask bytes of a sample (RFC 9001 5.4.3, 5.4.4): byte 0 for the
// first byte's low bits, bytes 1..4 (*pn_mask, byte k + 1 in bits 8k..8k+7)
// for the packet-number field.  hp, L: as dtls_mask_words' sn and L.
template <int MASK, class LDS>
__device__ __forceinline__ uint32_t quic_mask5(uint4 sample, const uint32_t *hp, const LDS &L,
                                               uint32_t *pn_mask) {
  uint32_t next;
  const uint32_t m = dtls_mask_words<MASK>(sample, hp, L, &next);
  *pn_mask = (m >> 8) | (next << 24);
  return m & 0xffu;
}

// The first byte's protected bits: four of a long header, five of a short one.
__device__ __forceinline__ uint32_t quic_first_byte_bits(uint32_t b0) {
  return (b0 & 0x80) ? 0x0fu : 0x1fu;
}

// RFC 9000 A.3: the packet number whose low 8 n bits are `truncated` closest
// to `expected`, never above 2^62 - 1.
__host__ __device__ inline uint64_t quic_decode_pn(uint64_t expected, uint64_t truncated, uint32_t n) {
  const uint64_t win = uint64_t(1) << (8 * n), hwin = win / 2;
  uint64_t cand = (expected & ~(win - 1)) | truncated;
  if (cand + hwin <= expected && cand < (uint64_t(1) << 62) - win)
    cand += win;
  else if (cand > expected + hwin && cand >= win)
    cand -= win;
  return cand;
}

// What both directions leave for the bulk kernels.
__device__ __forceinline__ void quic_describe(const QuicPrepare &p, uint64_t i, const QuicPacket &k,
                                              bool ok, uint32_t hdr_len, uint64_t body_len,
                                              const TlsIv &iv, uint64_t pn) {
  p.body_offsets[i] = k.off + (ok ? hdr_len : 0u);
  p.body_lengths[i] = ok ? body_len : 0;
  p.ad_lengths[i] = ok ? hdr_len : 0u;
  p.valid[i] = ok ? 1 : 0;
  dtls_xor_nonce(p.nonces + 12 * i, iv, pn);
}

// Seal: packet i with packet number pn.  The header goes to `out` with the
// length bits and the packet-number field filled in; nothing else of it
// changes.
__device__ __forceinline__ void quic_seal_packet(const QuicPrepare &p, uint64_t i, uint64_t pn,
                                                 const TlsIv &iv) {
  const QuicPacket k = quic_packet(p.offsets, p.lengths, p.packet_stride, p.packet_len,
                                   p.pn_offsets, p.pn_offset, i);
  const uint32_t n = p.pn_lengths ? p.pn_lengths[i] : p.pn_length;
  const uint64_t hdr = (uint64_t)k.pn_off + n;
  // (n + payload >= 4: the sample must end within the tag, RFC 9001 5.4.2.)
  const bool ok = n >= 1 && n <= 4 && k.pn_off != 0 && hdr <= k.len && k.len - k.pn_off >= 4;
  if (p.packet_numbers) p.packet_numbers[i] = pn;
  if (ok) {
    const uint8_t *src = p.in + k.off;
    uint8_t *dst = p.out + k.off;
    if (dst != src)
      for (uint32_t b = 1; b < k.pn_off; b++) dst[b] = src[b];
    dst[0] = (uint8_t)((src[0] & 0xfc) | (n - 1));
    for (uint32_t b = 0; b < n; b++) dst[k.pn_off + b] = (uint8_t)(pn >> (8 * (n - 1 - b)));
  }
  quic_describe(p, i, k, ok, (uint32_t)hdr, k.len - hdr, iv, pn);
}

// Open: packet i as received.  expected: the context's when the batch starts
// (every packet of a batch is decoded against it).
template <int MASK, class LDS>
__device__ __forceinline__ void quic_open_packet(const QuicPrepare &p, uint64_t i, const TlsIv &iv,
                                                 uint64_t expected, const uint32_t *hp,
                                                 const LDS &L) {
  const QuicPacket k = quic_packet(p.offsets, p.lengths, p.packet_stride, p.packet_len,
                                   p.pn_offsets, p.pn_offset, i);
  const bool ok = k.pn_off != 0 && k.len >= (uint64_t)k.pn_off + 20;  // room for the sample
  uint32_t hdr = 0;
  uint64_t pn = 0;
  if (ok) {
    const uint8_t *src = p.in + k.off;
    uint8_t *dst = p.out + k.off;
    uint32_t pn_mask;
    const uint32_t m0 = quic_mask5<MASK>(load_partial(src + k.pn_off + 4, 16), hp, L, &pn_mask);
    const uint32_t b0 = src[0];
    const uint32_t u0 = b0 ^ (m0 & quic_first_byte_bits(b0));
    const uint32_t n = (u0 & 3) + 1;
    uint64_t truncated = 0;
    for (uint32_t b = 0; b < n; b++)
      truncated = (truncated << 8) | (src[k.pn_off + b] ^ ((pn_mask >> (8 * b)) & 0xff));
    pn = quic_decode_pn(expected, truncated, n);
    hdr = k.pn_off + n;
    if (dst != src)
      for (uint32_t b = 1; b < k.pn_off; b++) dst[b] = src[b];
    dst[0] = (uint8_t)u0;
    for (uint32_t b = 0; b < n; b++) dst[k.pn_off + b] = (uint8_t)(truncated >> (8 * (n - 1 - b)));
    store16_any(p.tags + 16 * i, load_partial(src + k.len - 16, 16));
  }
  if (p.header_lengths) p.header_lengths[i] = hdr;
  if (p.packet_numbers) p.packet_numbers[i] = pn;
  p.pns[i] = pn;
  quic_describe(p, i, k, ok, hdr, ok ? k.len - hdr - 16 : 0, iv, pn);
}

// After a seal, packet i: the tag to the packet's end and the mask onto the
// header.  The sample is 16 bytes of ciphertext ++ tag from 4 bytes after the
// start of the packet-number field: it may straddle them or lie in the tag.
template <int MASK, class LDS>
__device__ __forceinline__ void quic_protect_packet(uint8_t *pkt, uint64_t len, uint64_t hdr,
                                                    uint64_t body_len, const uint8_t *tag,
                                                    const uint32_t *hp, const LDS &L) {
  const uint32_t n = (pkt[0] & 3) + 1;
  const uint64_t skip = 4 - n;  // of the body, before the sample
  uint32_t pn_mask;
  const uint32_t m0 =
      quic_mask5<MASK>(dtls_sample(pkt + hdr + skip, body_len - skip, tag), hp, L, &pn_mask);
  store_partial(pkt + len, load16_any(tag), 16);
  const uint32_t b0 = pkt[0];
  pkt[0] = (uint8_t)(b0 ^ (m0 & quic_first_byte_bits(b0)));
  for (uint32_t b = 0; b < n; b++) pkt[hdr - n + b] ^= (uint8_t)(pn_mask >> (8 * b));
}

}  // namespace
}  // namespace bssl_amd

#endif
