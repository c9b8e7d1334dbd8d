// dtls_prepare.h -- the per-record body of the DTLS record layer's prepare
// step (dtls.hip: dtls_prepare_kernel, one direction of one epoch), one
// __device__ function as tls_prepare.h has for TLS, so that a prepare kernel
// over many associations (dtls_set.hip) shares it: the differences are in what
// the caller passes (the epoch, the sequence number, the fixed IV, the window's
// maximum, the record-number key).
//
// Reference (one record per call): dtls_seal_record / dtls_open_record
// (ssl/dtls_record.cc:481-584, 292-425), SSLAEADContext (ssl/ssl_aead_ctx.cc:
// 207-380), the record-number encrypters (ssl/tls13_enc.cc:237-298) and
// reconstruct_seqnum (dtls_record.cc:92-120); RFC 6347 4.1, RFC 9147 4 - 4.2.3.
#ifndef BSSL_AMD_DTLS_PREPARE_H
#define BSSL_AMD_DTLS_PREPARE_H

#include <type_traits>

#include "internal.h"
#include "chacha_block.h"
#include "iov_dev.h"  // (before rec_blocks.h: mask_block)
#include "rec_blocks.h"
#include "tls_prepare.h"

namespace bssl_amd {
namespace {

constexpr bool dtls_mask_is_aes(int mask) { return mask == kDtlsMaskAes128 || mask == kDtlsMaskAes256; }

// Host: calls f with the DtlsMask as a compile-time constant, for the launchers
// of the kernels that are instantiated per mask.
template <class F>
void with_mask(int mask, F &&f) {
  switch (mask) {
    case kDtlsMaskAes128: f(std::integral_constant<int, kDtlsMaskAes128>{}); break;
    case kDtlsMaskAes256: f(std::integral_constant<int, kDtlsMaskAes256>{}); break;
    case kDtlsMaskChaCha: f(std::integral_constant<int, kDtlsMaskChaCha>{}); break;
    default: f(std::integral_constant<int, kDtlsMaskNone>{}); break;
  }
}

// The first 16 bytes of fragment || tag (RFC 9147 4.2.3's sample), as
// little-endian words: a fragment shorter than 16 bytes continues in the tag
// slot, and no byte past the fragment's last dword is read from the body.
__device__ __forceinline__ uint4 dtls_sample(const uint8_t *frag, uint64_t frag_len,
                                             const uint8_t *tag) {
  const uint32_t n1 = frag_len < 16 ? (uint32_t)frag_len : 16u;
  const uint4 a = load_partial(frag, n1);
  if (n1 == 16) return a;
  const uint4 b = load_partial(tag, 16 - n1);
  const uint4 s = bytes_at(make_uint4(0, 0, 0, 0), b, 16 - n1);  // b << 8 n1
  return make_uint4(a.x | s.x, a.y | s.y, a.z | s.z, a.w | s.w);
}

// The first four mask bytes of a sample (byte k: bits 8k..8k+7) and, in *next,
// the four after them (QUIC's mask has five, quic_prepare.h).  sn: the
// record-number key as DtlsState holds it -- wave-uniform for one association,
// the lane's own for a set (AES: its LDS slot, lane_frame.h); L: the
// workgroup's T-table (AES), unused otherwise.
template <int MASK, class LDS>
__device__ __forceinline__ uint32_t dtls_mask_words(uint4 sample, const uint32_t *sn, const LDS &L,
                                                    uint32_t *next) {
  if constexpr (dtls_mask_is_aes(MASK)) {
    // AES-ECB(sn_key, sample) (tls13_enc.cc:243-251).
    uint4 s[1] = {sample};
    aes_n<MASK == kDtlsMaskAes128 ? 10 : 14, 1>(s, sn, L);
    *next = s[0].y;
    return s[0].x;
  } else if constexpr (MASK == kDtlsMaskChaCha) {
    // The first keystream bytes of ChaCha20 (RFC 8439 2.3) with block counter
    // le32(sample[0..4)) and nonce sample[4..16) (tls13_enc.cc:279-293).
    uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
    for (int k = 0; k < 8; k++) in[4 + k] = sn[k];
    in[12] = sample.x;
    in[13] = sample.y;
    in[14] = sample.z;
    in[15] = sample.w;
    uint32_t head[4];
    chacha20_block_head(in, head);
    *next = head[1];
    return head[0];
  } else {
    *next = 0;
    return 0;
  }
}

// Mask bytes 0 (bits 0..7) and 1 (bits 8..15) of a sample.
template <int MASK, class LDS>
__device__ __forceinline__ uint32_t dtls_mask16(uint4 sample, const uint32_t *sn, const LDS &L) {
  uint32_t next;
  return dtls_mask_words<MASK>(sample, sn, L, &next) & 0xffffu;
}

// reconstruct_seqnum (dtls_record.cc:92-120): the value congruent to `wire`
// modulo mask + 1 (0xff or 0xffff) that is closest to max_seq + 1, the larger
// one on a tie, never negative and never above 2^48 - 1.
__host__ __device__ inline uint64_t dtls_reconstruct_seqnum(uint32_t wire, uint64_t mask,
                                                            uint64_t max_seq) {
  const uint64_t next = max_seq + 1, step = mask + 1;
  const uint64_t diff = ((uint64_t)wire - next) & mask;
  uint64_t s = next + diff;
  if (s > kDtlsMaxSequence || (diff > step / 2 && s >= step)) s -= step;
  return s;
}

// be64(v) XORed into (xor_nonce) or placed after (else) the fixed IV.
__device__ __forceinline__ void dtls_xor_nonce(uint8_t *nonce, const TlsIv &iv, uint64_t v) {
  for (int k = 0; k < 12; k++)
    nonce[k] = (uint8_t)(iv.byte(k) ^ (k >= 4 ? (uint8_t)(v >> (8 * (11 - k))) : 0));
}

// Seal: record i with sequence number seq.  valid[i] comes from the TLS 1.3
// pre-pass (tls_pad.hip) in DTLS 1.3, whose lengths are the fragment lengths;
// in DTLS 1.2 it is written here.
__device__ __forceinline__ void dtls_seal_record(const DtlsPrepare &p, uint64_t i, uint32_t epoch,
                                                 uint64_t seq, const TlsIv &iv) {
  const uint64_t len = p.lengths ? p.lengths[i] : p.record_len;
  const uint64_t combined = ((uint64_t)epoch << 48) | seq;
  uint8_t *pre = p.prefix + p.prefix_len * i;
  uint8_t *nonce = p.nonces + 12 * i;
  uint8_t *ad = p.ad + p.ad_stride * i;
  if (p.record_numbers) p.record_numbers[i] = combined;
  bool ok;
  if (p.dtls13) {
    // The unified header with a 16-bit sequence number and a length (RFC 9147
    // 4; dtls_record.cc:520-540), also the additional data; the nonce takes
    // the sequence number alone (dtls_aead_sequence, :71-78).
    ok = p.valid[i] != 0;
    const uint64_t ctlen = len + 16;
    const uint8_t hdr[5] = {(uint8_t)(0x2c | (epoch & 3)), (uint8_t)(seq >> 8), (uint8_t)seq,
                            (uint8_t)(ctlen >> 8), (uint8_t)ctlen};
    for (int k = 0; k < 5; k++) {
      pre[k] = ok ? hdr[k] : 0;
      ad[k] = hdr[k];
    }
    dtls_xor_nonce(nonce, iv, seq);
    return;
  }
  // DTLS 1.2 (RFC 6347 4.1; dtls_record.cc:541-556): the header carries the
  // record number, the AEAD takes epoch || sequence as its sequence number.
  ok = len <= kTlsMaxPlainLen;
  const uint8_t type = p.types ? p.types[i] : p.type;
  const uint32_t explicit_len = p.prefix_len - 13;
  const uint64_t ctlen = explicit_len + len + 16;
  if (p.xor_nonce) {
    dtls_xor_nonce(nonce, iv, combined);
  } else {
    for (int k = 0; k < 4; k++) nonce[k] = iv.byte(k);
    for (int k = 0; k < 8; k++) nonce[4 + k] = (uint8_t)(combined >> (8 * (7 - k)));
  }
  for (int k = 0; k < 8; k++) ad[k] = (uint8_t)(combined >> (8 * (7 - k)));
  ad[8] = type;
  ad[9] = 0xfe;
  ad[10] = 0xfd;
  ad[11] = (uint8_t)(len >> 8);
  ad[12] = (uint8_t)len;
  uint8_t hdr[21];
  hdr[0] = type;
  hdr[1] = 0xfe;
  hdr[2] = 0xfd;
  for (int k = 0; k < 8; k++) hdr[3 + k] = ad[k];
  hdr[11] = (uint8_t)(ctlen >> 8);
  hdr[12] = (uint8_t)ctlen;
  for (int k = 0; k < 8; k++) hdr[13 + k] = ad[k];  // the explicit nonce (AES-GCM)
  for (uint32_t k = 0; k < p.prefix_len; k++) pre[k] = ok ? hdr[k] : 0;
  if (p.out_lengths) p.out_lengths[i] = ok ? len : 0;
  if (!ok) p.valid[i] = 0;
}

// Open: record i as received.  max_seq: the window's maximum when the batch
// starts (every record of a batch is reconstructed against it); sn, L: see
// dtls_mask16.  Writes valid[i], seqs[i] and record_numbers[i] for every
// record.
template <int MASK, class LDS>
__device__ __forceinline__ void dtls_open_record(const DtlsPrepare &p, uint64_t i, uint32_t epoch,
                                                 const TlsIv &iv, uint64_t max_seq,
                                                 const uint32_t *sn, const LDS &L) {
  const uint64_t len = p.lengths ? p.lengths[i] : p.record_len;
  const uint8_t *pre = p.prefix + p.prefix_len * i;
  uint8_t *nonce = p.nonces + 12 * i;
  uint8_t *ad = p.ad + p.ad_stride * i;
  uint64_t s = 0;
  bool ok;
  if (p.dtls13) {
    // parse_dtls13_record (dtls_record.cc:170-230): 0 0 1 C S L E E.
    const uint32_t b0 = pre[0];
    const uint32_t seq_len = (b0 & 0x08) ? 2 : 1, has_len = (b0 & 0x04) ? 1 : 0;
    const uint32_t hdr_len = 1 + seq_len + 2 * has_len;
    const uint32_t w0 = pre[1], w1 = pre[2], w2 = pre[3], w3 = pre[4];
    const uint64_t stated = seq_len == 2 ? (w2 << 8) | w3 : (w1 << 8) | w2;
    ok = (b0 & 0xe0) == 0x20 && (b0 & 0x10) == 0 && (b0 & 3) == (epoch & 3) &&
         len >= 1 && len <= kTlsMaxPlainLen + 1 &&
         (!has_len || (stated == len + 16 && stated <= kTlsMaxEncryptedLen));
    uint32_t m = 0;
    if (ok) {
      const uint64_t off = p.offsets ? p.offsets[i] : i * p.record_stride;
      m = dtls_mask16<MASK>(dtls_sample(p.body + off, len, p.suffix + 16 * i), sn, L);
    }
    const uint32_t u0 = w0 ^ (m & 0xff), u1 = w1 ^ (m >> 8);
    s = seq_len == 2 ? dtls_reconstruct_seqnum((u0 << 8) | u1, 0xffff, max_seq)
                     : dtls_reconstruct_seqnum(u0, 0xff, max_seq);
    // The additional data: the header as received, its sequence bytes unmasked.
    ad[0] = (uint8_t)b0;
    ad[1] = (uint8_t)u0;
    ad[2] = seq_len == 2 ? (uint8_t)u1 : (uint8_t)w1;
    ad[3] = (uint8_t)w2;
    ad[4] = (uint8_t)w3;
    p.ad_lengths[i] = hdr_len;
    dtls_xor_nonce(nonce, iv, s);
  } else {
    // dtls_open_record's DTLSPlaintext-shaped header (:232-262, 316-345).
    const uint32_t explicit_len = p.prefix_len - 13;
    const uint32_t type = pre[0];
    const uint32_t version = ((uint32_t)pre[1] << 8) | pre[2];
    const uint32_t hdr_epoch = ((uint32_t)pre[3] << 8) | pre[4];
    for (int k = 0; k < 6; k++) s = (s << 8) | pre[5 + k];
    const uint64_t stated = ((uint64_t)pre[11] << 8) | pre[12];
    ok = (type & 0xe0) != 0x20 && version == 0xfefd && hdr_epoch == epoch &&
         len <= kTlsMaxPlainLen && stated == explicit_len + len + 16 &&
         stated <= kTlsMaxEncryptedLen;
    const uint64_t combined = ((uint64_t)epoch << 48) | s;
    if (p.types_out) p.types_out[i] = (uint8_t)type;
    if (p.xor_nonce) {
      dtls_xor_nonce(nonce, iv, combined);
    } else {  // the explicit nonce travels in the record
      for (int k = 0; k < 4; k++) nonce[k] = iv.byte(k);
      for (int k = 0; k < 8; k++) nonce[4 + k] = pre[13 + k];
    }
    for (int k = 0; k < 8; k++) ad[k] = (uint8_t)(combined >> (8 * (7 - k)));
    ad[8] = (uint8_t)type;
    ad[9] = 0xfe;
    ad[10] = 0xfd;
    ad[11] = (uint8_t)(len >> 8);
    ad[12] = (uint8_t)len;
  }
  p.valid[i] = ok ? 1 : 0;
  p.seqs[i] = s;
  if (p.record_numbers) p.record_numbers[i] = ok ? ((uint64_t)epoch << 48) | s : 0;
}

// Record i of a batch in epoch `epoch` (one association: DtlsPrepare::epoch; a
// set: the slot's): seq is read on seal, max_seq / sn / L on open.
template <int MASK, class LDS>
__device__ __forceinline__ void dtls_prepare_record(const DtlsPrepare &p, uint64_t i,
                                                    uint32_t epoch, uint64_t seq, const TlsIv &iv,
                                                    uint64_t max_seq, const uint32_t *sn,
                                                    const LDS &L) {
  if (p.open)
    dtls_open_record<MASK>(p, i, epoch, iv, max_seq, sn, L);
  else
    dtls_seal_record(p, i, epoch, seq, iv);
}

}  // namespace
}  // namespace bssl_amd

#endif
