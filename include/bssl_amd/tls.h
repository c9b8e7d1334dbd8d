/* bssl_amd/tls.h -- TLS record protection over device batches: the record
 * layer that calls the AEAD path.
 *
 * BSSL_AMD_TLS_AEAD is one direction of a TLS 1.2 / 1.3 connection with an
 * AEAD cipher suite -- the analogue of the reference's SSLAEADContext
 * (ssl/internal.h; ssl/ssl_aead_ctx.cc:44-123, 207-409) -- and a batch of
 * records is what do_seal_record / tls_open_record (ssl/tls_record.cc:266-317,
 * 183-236) do per record, with write/read sequence numbers seq, seq+1, ...
 *
 * Record layout (scatter, as SealScatter's out_prefix / out / out_suffix):
 *   prefix[i]  prefix_len bytes: the 5-byte record header, then for TLS 1.2
 *              AES-GCM the 8-byte explicit nonce
 *   body       record i's plaintext / ciphertext at in/out + offsets[i]
 *              (or i * record_stride), lengths[i] (or record_len) bytes
 *   suffix[i]  suffix_len bytes: for TLS 1.3 the sealed inner content type,
 *              then the 16-byte tag
 * so header ++ prefix-rest ++ body ++ suffix is the wire record.  TLS 1.3
 * records are sealed without padding; open expects unpadded records (the
 * inner type is the byte after the body) and returns it in types[i].  Padded
 * TLS 1.3 records (RFC 8446 5.4) have calls and a layout of their own:
 * BSSL_AMD_TLS_AEAD_seal_tls13_padded_device and
 * BSSL_AMD_TLS_AEAD_open_tls13_padded_device below.
 *
 * The TLS 1.1 / 1.2 AES-CBC-HMAC suites (BSSL_AMD_TLS_AEAD_new_cbc; the
 * reference's SSLAEADContext with a MAC key, ssl_aead_ctx.cc:95-114) have
 * another layout.  With mac_len 20 (SHA-1) or 32 (SHA-256) and, for a
 * plaintext of len bytes, pad_len = 16 - (len + mac_len) mod 16:
 *   prefix[i]  21 bytes: type, be16(version), be16(16 + len + mac_len +
 *              pad_len), then the 16-byte explicit IV
 *   body       seal: the first len bytes of the CBC output.  Open: the whole
 *              fragment after the IV (body, MAC and padding together, a
 *              multiple of 16 bytes) at in + offsets[i], lengths[i] bytes; the
 *              whole decryption goes to out + offsets[i] and the plaintext
 *              length to out_lengths[i]
 *   suffix[i]  seal: suffix_len bytes (the AEAD's overhead, 36 or 48), of
 *              which the first mac_len + pad_len hold the rest of the CBC
 *              output and the others are zero; prefix ++ body ++
 *              suffix[0, mac_len + pad_len) is the wire record.  Open: unused,
 *              may be NULL
 * and the additional data is be64(seq) ++ type ++ be16(version), 11 bytes
 * (open: the type of the received header).
 */
#ifndef BSSL_AMD_TLS_H
#define BSSL_AMD_TLS_H

#include "bssl_amd/aead.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSSL_AMD_TLS1_1_VERSION 0x0302
#define BSSL_AMD_TLS1_2_VERSION 0x0303
#define BSSL_AMD_TLS1_3_VERSION 0x0304

typedef struct bssl_amd_tls_aead_st BSSL_AMD_TLS_AEAD;

/* SSLAEADContext::Create for an AEAD cipher suite (mac_key empty):
 * `aead` is EVP_aead_aes_128_gcm(), EVP_aead_aes_256_gcm() or
 * EVP_aead_chacha20_poly1305(); AES-GCM seal contexts use the reference's
 * nonce-checking tls12 / tls13 variants (ssl_cipher_get_evp_aead,
 * ssl/ssl_cipher.cc).  fixed_iv: 4 bytes for TLS 1.2 AES-GCM, 12 otherwise.
 * `seq` is the sequence number of the first record (TLS 1.3 traffic keys
 * start at 0, which the tls13 AEAD's nonce check relies on, e_aes.cc.inc:
 * 1181-1185).  Returns NULL on error; any other AEAD (AES-GCM-SIV, XChaCha,
 * AES-CCM, AES-EAX: the reference's TLS stack has no such suites) is rejected
 * with CIPHER_R_UNSUPPORTED_KEY_SIZE, the AES-CTR-HMAC-SHA256 AEADs and the
 * TLS AES-CBC-HMAC AEADs (EVP_aead_aes_*_cbc_sha*_tls: the CBC suites have
 * split keys and no fixed IV, see BSSL_AMD_TLS_AEAD_new_cbc) with
 * CIPHER_R_CTRL_NOT_IMPLEMENTED. */
BSSL_AMD_EXPORT BSSL_AMD_TLS_AEAD *BSSL_AMD_TLS_AEAD_new(
    enum evp_aead_direction_t direction, uint16_t version, const EVP_AEAD *aead,
    const uint8_t *key, size_t key_len, const uint8_t *fixed_iv, size_t fixed_iv_len,
    uint64_t seq);
/* SSLAEADContext::Create for a CBC cipher suite of TLS 1.1 or 1.2 (explicit
 * IV; ssl_aead_ctx.cc:95-114): `aead` is EVP_aead_aes_128_cbc_sha1_tls(),
 * EVP_aead_aes_256_cbc_sha1_tls() or EVP_aead_aes_128_cbc_sha256_tls(), the
 * context EVP_AEAD_CTX_init_with_direction(aead, mac_key ++ enc_key, tag
 * length 0, direction).  `version` (0x0302 or 0x0303) is also the record
 * version of the header and of the additional data.  There is no fixed IV:
 * that is the TLS 1.0 implicit-IV form, which is not supported.  Checked before
 * any GPU call: another version, a NULL aead or key is
 * ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED; another AEAD CIPHER_R_CTRL_NOT_IMPLEMENTED;
 * mac_key_len other than the MAC size (20 or 32), or mac_key_len + enc_key_len
 * other than EVP_AEAD_key_length(aead), CIPHER_R_UNSUPPORTED_KEY_SIZE.
 * prefix_len is 21, suffix_len EVP_AEAD_max_overhead(aead) (36 or 48).
 *
 * A sealing context draws a 32-byte key from getrandom(2) (failure:
 * ERR_R_INTERNAL_ERROR) for the explicit IVs it generates: the IV of sequence
 * number s is bytes 0..15 of the ChaCha20 block (RFC 8439 2.3) of that key
 * with block counter (uint32)s and nonce words (uint32)(s >> 32), 0, 0 --
 * unpredictable without the key, one block per sequence number.  The key
 * stays in the host object and is zeroed by BSSL_AMD_TLS_AEAD_free. */
BSSL_AMD_EXPORT BSSL_AMD_TLS_AEAD *BSSL_AMD_TLS_AEAD_new_cbc(
    enum evp_aead_direction_t direction, uint16_t version, const EVP_AEAD *aead,
    const uint8_t *enc_key, size_t enc_key_len, const uint8_t *mac_key, size_t mac_key_len,
    uint64_t seq);
BSSL_AMD_EXPORT void BSSL_AMD_TLS_AEAD_free(BSSL_AMD_TLS_AEAD *t);
BSSL_AMD_EXPORT size_t BSSL_AMD_TLS_AEAD_prefix_len(const BSSL_AMD_TLS_AEAD *t);
BSSL_AMD_EXPORT size_t BSSL_AMD_TLS_AEAD_suffix_len(const BSSL_AMD_TLS_AEAD *t);
/* The sequence number the next record will use. */
BSSL_AMD_EXPORT uint64_t BSSL_AMD_TLS_AEAD_sequence(const BSSL_AMD_TLS_AEAD *t);

typedef struct {
  size_t num_records;
  const uint8_t *in; /* device */
  uint8_t *out;      /* device, may equal in */
  const uint64_t *offsets; /* device, or NULL: i * record_stride */
  const uint64_t *lengths; /* device, or NULL: record_len */
  uint64_t record_stride;
  uint64_t record_len;
  /* Seal: the content type of record i (device, or NULL: `type` for all).
   * Open: receives the inner type (TLS 1.3) or the header type (TLS 1.2). */
  uint8_t *types;
  uint8_t type;
  uint8_t *prefix; /* device, prefix_len bytes per record */
  uint8_t *suffix; /* device, suffix_len bytes per record */
  uint8_t *status; /* device, 1 byte per record (1 = sealed / authentic), or NULL */
  /* The two fields below are read for CBC contexts (BSSL_AMD_TLS_AEAD_new_cbc)
   * only: a caller of the AEAD suites compiled against the structure without
   * them keeps working. */
  /* CBC open: receives record i's plaintext length, 0 for a failed record
   * (device).  Required for CBC open. */
  uint64_t *out_lengths;
  /* CBC seal: the explicit IVs to use, 16 bytes per record (device), or NULL:
   * generated (BSSL_AMD_TLS_AEAD_new_cbc).  Ignored on open. */
  const uint8_t *explicit_ivs;
} BSSL_AMD_TLS_RECORDS;

/* Seal (open) num_records records with sequence numbers sequence() ..
 * sequence() + n - 1 and advance the sequence by n.  A record that fails
 * (plaintext > 2^14 bytes, a rejected nonce, a bad tag) has status 0 and
 * zeroed outputs; it still consumes its sequence number.  Returns 0 (nothing
 * launched, error queued) when the sequence number would wrap
 * (tls_record.cc:305-308) or on argument errors.  Synchronises the stream
 * for AES-GCM seal (the nonce state, see EVP_AEAD_CTX_seal_batch_device); a
 * CBC seal, with generated IVs too, only enqueues work.
 *
 * CBC open (tls_open_record + SSLAEADContext::Open): prefix[i] holds the
 * received header and IV; the header type goes to types[i] when `types` is
 * given.  A record fails alone (status 0, lengths[i] zero bytes of output,
 * out_lengths[i] 0) when the header's version is not the context's
 * (tls_record.cc:117-130), its length is not 16 + lengths[i], 16 + lengths[i]
 * exceeds 16704 (SSL3_RT_MAX_ENCRYPTED_LENGTH, :133), lengths[i] is no
 * multiple of 16 or below mac_len + 1, the padding or the MAC is wrong, or the
 * plaintext is longer than 2^14 bytes (:204-209).  out_lengths == NULL is an
 * argument error (ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED, nothing launched). */
BSSL_AMD_EXPORT int BSSL_AMD_TLS_AEAD_seal_records_device(BSSL_AMD_TLS_AEAD *t,
                                                          const BSSL_AMD_TLS_RECORDS *r,
                                                          void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_TLS_AEAD_open_records_device(BSSL_AMD_TLS_AEAD *t,
                                                          const BSSL_AMD_TLS_RECORDS *r,
                                                          void *hip_stream);

/* ---- TLS 1.3 record padding (RFC 8446 5.4) --------------------------------
 *
 * A TLS 1.3 peer may append zero bytes after the inner content type, and a
 * receiver strips them (tls_record.cc:198-229).  The padded calls take the
 * fragment -- the encrypted TLSInnerPlaintext, content || type || zeros -- in
 * one piece:
 *   prefix[i]  the 5-byte header
 *   body       the whole fragment at in/out + offsets[i]
 *   suffix[i]  the 16-byte tag alone, stride BSSL_AMD_TLS13_TAG_LEN (not
 *              suffix_len(), which stays the unpadded calls' 17)
 * so prefix ++ body ++ suffix is the wire record.  Contexts and sets of TLS
 * 1.3 serve both these and the unpadded calls, on one sequence of numbers.
 *
 * Seal: lengths[i] is the content length L.  The fragment has F = L + 1 + P
 * bytes: P = pad_lengths[i]; or, with pad_block B > 1, F = min(B * ceil((L +
 * 1) / B), 2^14 + 1); or P = 0 (also for pad == NULL).  The caller leaves room
 * for F bytes at out + offsets[i]; the ciphertext of content || type || P
 * zeros goes there (out may equal in; if not, the content is copied), the
 * header says F + 16 (type 23, version 0x0303; it is the additional data), the
 * nonce is the unpadded call's, and out_lengths[i], when given, receives F.  A
 * record fails alone -- status 0, tag and content bytes zeroed, nothing
 * written past out + offsets[i] + L, out_lengths[i] 0, its sequence number
 * consumed like an oversize record's -- when L > 2^14, when F > 2^14 + 1 (RFC
 * 8446 5.4; what a reader enforces, tls_record.cc:204-209), or when its type is
 * 0, which a reader would take for padding.
 *
 * Open: lengths[i] is the received fragment length F (the header's length
 * minus 16) and suffix[i] the tag.  out_lengths and types are required
 * (ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED, nothing launched).  With k the index of
 * the last non-zero byte of the decrypted fragment, types[i] = out[offsets[i]
 * + k] and out_lengths[i] = k; the bytes from k on stay as decrypted.  A record
 * fails alone -- status 0, F zero bytes of output, out_lengths[i] 0, types[i]
 * 0, its sequence number consumed -- when the header's type is not 23
 * (tls_record.cc:214), its version not 0x0303 (:117-130), its length not F + 16
 * or F + 16 > 16704 (:133), F > 2^14 + 1 (:204-209), F = 0, the tag is bad, or
 * the whole fragment is zero (:220-225).
 *
 * Argument errors, all before any GPU call: a context or set that is not TLS
 * 1.3, CBC contexts included (ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED); the wrong
 * direction (CIPHER_R_INVALID_OPERATION); NULL in, out, prefix or suffix with
 * records present; a sequence number that would wrap.  The calls only enqueue
 * work, but the one-connection AES-GCM seal synchronises the stream for its
 * nonce state like the unpadded one.  In a set the run rules, the failures
 * that consume no sequence number and the zeroed prefix on seal are those of
 * the unpadded set calls (below). */
#define BSSL_AMD_TLS13_TAG_LEN 16
typedef struct {
  const uint32_t *pad_lengths; /* device, zero bytes to add to record i; or NULL */
  uint32_t pad_block;          /* read when pad_lengths == NULL; 0 or 1: no padding */
} BSSL_AMD_TLS13_PADDING;

BSSL_AMD_EXPORT int BSSL_AMD_TLS_AEAD_seal_tls13_padded_device(
    BSSL_AMD_TLS_AEAD *t, const BSSL_AMD_TLS_RECORDS *r,
    const BSSL_AMD_TLS13_PADDING *pad /* NULL: none */, void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_TLS_AEAD_open_tls13_padded_device(BSSL_AMD_TLS_AEAD *t,
                                                               const BSSL_AMD_TLS_RECORDS *r,
                                                               void *hip_stream);

/* ---- Connection sets: one record batch across many connections ------------
 *
 * BSSL_AMD_TLS_SET is one direction of up to num_connections connections of
 * ONE cipher suite.  Every slot holds what a BSSL_AMD_TLS_AEAD holds -- a key,
 * a fixed IV and the next sequence number -- but on the device, so that one
 * call protects a batch that mixes the records of many connections and only
 * enqueues work.
 *
 * Records [run_start[j], run_start[j+1]) of a batch belong to connection
 * c = run_connection[j] (per-connection send queues, concatenated).  Record i
 * of run j gets the sequence number S[c] + (i - run_start[j]), where S[c] is
 * the connection's next sequence number at the point of the stream where the
 * call's work runs; afterwards S[c] has advanced by the run's record count.
 * Prefix, body, suffix, status and returned type of every record are byte for
 * byte what BSSL_AMD_TLS_AEAD_new(direction, version, aead, key_c, iv_c, S[c])
 * produces for that connection's records in order.
 *
 * Seal and open only enqueue work on hip_stream: they never synchronise it,
 * not for AES-GCM either.  The state of a set lives in stream order, so all
 * calls of one set must be issued on one stream, or be ordered by the caller
 * (events) as if they were.
 *
 * A record that fails has status 0 and the zeroed outputs the one-connection
 * layer leaves; the other records of the batch are untouched.
 *   - Seal: plaintext over 2^14 bytes; open: bad tag.  The record consumes
 *     its sequence number, as in the one-connection layer.
 *   - The record's sequence number would be 2^64 - 1, or past it
 *     (tls_record.cc:302-306; e_aes.cc.inc:1087).  S[c] saturates at 2^64 - 1:
 *     that record and all later ones of the connection fail.
 *   - run_connection[j] is out of range, or the slot is unset.
 *   - The connection already has an earlier non-empty run in this call: two
 *     runs would both start from S[c].  The lowest j wins, the records of the
 *     later runs fail and S[c] advances by the winning run only.
 *   - The record index is not inside the run found for it (a malformed
 *     run_start).  Nothing outside the batch's arrays is read or written.
 * The records of the last four rules get no sequence number and consume none;
 * on seal their prefix is zeroed too (there is no header to write).
 *
 * One deliberate departure from the reference: its tls13 AES-GCM AEAD learns
 * its nonce mask from the first nonce and so only works for a context that
 * starts at sequence number 0 (e_aes.cc.inc:1181-1194).  A set does not run
 * the tls12 / tls13 nonce checks against host state: nothing but the set
 * advances a connection's counter, so its nonces increase strictly by
 * construction.  A slot may therefore be installed at any sequence number,
 * TLS 1.3 AES-GCM included -- which is what moving a live connection onto the
 * GPU needs.
 *
 * Out of scope: the CBC suites in a set; mixed suites in one set; more than
 * one run per connection per call. */
typedef struct bssl_amd_tls_set_st BSSL_AMD_TLS_SET;

/* The version / aead rules and codes of BSSL_AMD_TLS_AEAD_new (TLS 1.2 / 1.3;
 * AES-128-GCM, AES-256-GCM, ChaCha20-Poly1305; the AES-CTR-HMAC and CBC AEADs
 * CIPHER_R_CTRL_NOT_IMPLEMENTED); num_connections 0 or above 2^32 - 2 is
 * ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED.  All checks come before any GPU call.
 * All slots start unset. */
BSSL_AMD_EXPORT BSSL_AMD_TLS_SET *BSSL_AMD_TLS_SET_new(enum evp_aead_direction_t direction,
                                                       uint16_t version, const EVP_AEAD *aead,
                                                       size_t num_connections);
/* Waits for the device, zeroes the key material on it and frees it. */
BSSL_AMD_EXPORT void BSSL_AMD_TLS_SET_free(BSSL_AMD_TLS_SET *s);
BSSL_AMD_EXPORT size_t BSSL_AMD_TLS_SET_num_connections(const BSSL_AMD_TLS_SET *s);
BSSL_AMD_EXPORT size_t BSSL_AMD_TLS_SET_prefix_len(const BSSL_AMD_TLS_SET *s);
BSSL_AMD_EXPORT size_t BSSL_AMD_TLS_SET_suffix_len(const BSSL_AMD_TLS_SET *s);

/* (Re)key slots first .. first+n-1 from HOST arrays: n keys, n fixed IVs (4
 * bytes each for TLS 1.2 AES-GCM, 12 otherwise), n starting sequence numbers
 * (NULL: all 0).  Ordered on hip_stream with the set's batches: batches
 * enqueued before it use the old keys, batches after it the new.  The host
 * waits until the device has taken the staged key material (its host copies
 * are zeroed before the call returns), and so for the work enqueued before it
 * on hip_stream.  A slot range outside the set is
 * ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED. */
BSSL_AMD_EXPORT int BSSL_AMD_TLS_SET_set_connections(BSSL_AMD_TLS_SET *s, size_t first, size_t n,
                                                     const uint8_t *keys,
                                                     const uint8_t *fixed_ivs,
                                                     const uint64_t *seqs, void *hip_stream);
/* Unset slots (key material zeroed on the device, in stream order); their
 * records then fail.  Only enqueues work. */
BSSL_AMD_EXPORT int BSSL_AMD_TLS_SET_clear_connections(BSSL_AMD_TLS_SET *s, size_t first,
                                                       size_t n, void *hip_stream);
/* Copies the next sequence numbers of slots first..first+n-1 to HOST memory
 * (0 for an unset slot); synchronises hip_stream. */
BSSL_AMD_EXPORT int BSSL_AMD_TLS_SET_sequences(BSSL_AMD_TLS_SET *s, size_t first, size_t n,
                                               uint64_t *out, void *hip_stream);

typedef struct {
  BSSL_AMD_TLS_RECORDS records; /* layout exactly as for one connection;
                                   out_lengths / explicit_ivs are not read */
  size_t num_runs;              /* at most 2^32 - 2 */
  const uint32_t *run_connection; /* device, num_runs entries */
  const uint64_t *run_start; /* device, num_runs + 1 entries, non-decreasing,
                                run_start[0] = 0, run_start[num_runs] = num_records */
} BSSL_AMD_TLS_SET_RECORDS;

/* Seal (open) the batch; see above.  Returns 0 with nothing launched and an
 * error queued for argument errors: NULL pointers as for one connection,
 * num_runs == 0 with num_records != 0, missing run arrays, TLS 1.3 open
 * without `types`, the wrong direction (CIPHER_R_INVALID_OPERATION). */
BSSL_AMD_EXPORT int BSSL_AMD_TLS_SET_seal_records_device(BSSL_AMD_TLS_SET *s,
                                                         const BSSL_AMD_TLS_SET_RECORDS *r,
                                                         void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_TLS_SET_open_records_device(BSSL_AMD_TLS_SET *s,
                                                         const BSSL_AMD_TLS_SET_RECORDS *r,
                                                         void *hip_stream);

/* The TLS 1.3 padded form of the two calls above (see "TLS 1.3 record
 * padding"): r->records in the padded layout, out_lengths read as there. */
BSSL_AMD_EXPORT int BSSL_AMD_TLS_SET_seal_tls13_padded_device(BSSL_AMD_TLS_SET *s,
                                                              const BSSL_AMD_TLS_SET_RECORDS *r,
                                                              const BSSL_AMD_TLS13_PADDING *pad,
                                                              void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_TLS_SET_open_tls13_padded_device(BSSL_AMD_TLS_SET *s,
                                                              const BSSL_AMD_TLS_SET_RECORDS *r,
                                                              void *hip_stream);

/* ---- DTLS 1.2 and 1.3 record protection -----------------------------------
 *
 * BSSL_AMD_DTLS_AEAD is one direction of one epoch of one DTLS association:
 * dtls_seal_record / dtls_open_record (ssl/dtls_record.cc:481-584, 292-425)
 * for a batch of records.  What differs from TLS: a record's number travels in
 * its header, so records may arrive reordered, duplicated or forged, and an
 * opening context keeps the reference's 256-entry anti-replay window
 * (DTLSReplayBitmap, dtls_record.cc:29-57) -- on the device, so that both
 * calls only enqueue work on hip_stream, for AES-GCM too.  The state of a
 * context lives in stream order: issue all calls of one context on one stream,
 * or order them as if they were.
 *
 * The AEAD is the plain one, not the nonce-checking tls12 / tls13 variants:
 * the context generates its own sequence numbers, so its nonces rise strictly
 * by construction, and it may start at any `seq` -- the deliberate departure
 * from the reference that the connection sets document above.
 *
 * Wire record i = prefix[i] ++ body ++ suffix[i]; suffix[i] is the 16-byte
 * tag.  With combined = epoch << 48 | seq:
 *
 * DTLS 1.2 (RFC 6347 4.1).  prefix_len 13, or 21 for AES-GCM (the 8-byte
 * explicit nonce follows the header):
 *   header  type, be16(0xfefd), be16(epoch), be48(seq), be16(explicit + L + 16)
 *   body    L bytes
 *   AD      be64(combined) ++ type ++ fe fd ++ be16(L)
 *   nonce   AES-GCM: iv4 ++ be64(combined), whose last 8 bytes are the explicit
 *           nonce written on seal and read from the prefix on open;
 *           ChaCha20-Poly1305: iv12 XOR (0^4 ++ be64(combined))
 *
 * DTLS 1.3 (RFC 9147 4).  prefix_len 5.  The body is the whole fragment,
 * content ++ type ++ zeros, the layout of the TLS 1.3 padded calls:
 *   seal    lengths[i] is the content length L; the caller leaves room for
 *           L + 1 bytes at out + offsets[i] (no padding is added, as in the
 *           reference); out_lengths[i], when given, receives L + 1
 *   header  0x2c | (epoch & 3), be16(seq & 0xffff), be16(L + 1 + 16); it is the
 *           AD, with the sequence bytes in the clear
 *   nonce   iv12 XOR (0^4 ++ be64(seq)): the sequence number without the epoch
 *           (dtls_aead_sequence, dtls_record.cc:71-78)
 *   mask    after the AEAD, header bytes 1..2 are XORed with mask bytes 0..1
 *           (RFC 9147 4.2.3; ssl/tls13_enc.cc:237-298).  The sample is the
 *           first 16 bytes of body ++ tag.  AES suites: AES-ECB(sn_key,
 *           sample); ChaCha20: the first keystream bytes of ChaCha20 with key
 *           sn_key, block counter le32(sample[0..4)), nonce sample[4..16)
 *
 * Seal.  Record i gets sequence number sequence() + i and the context advances
 * by n.  Returns 0 with nothing launched when sequence() + n - 1 > 2^48 - 1
 * (HasNext, dtls_record.cc:500-505) or on argument errors: NULL in, out, prefix
 * or suffix with records present (ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED), the wrong
 * direction (CIPHER_R_INVALID_OPERATION).  A record fails alone and still
 * consumes its number -- status 0; body, tag and prefix zeroed; out_lengths[i]
 * 0 -- when L > 2^14, or in DTLS 1.3 when its type is 0.  record_numbers[i] =
 * combined is written for every record.
 *
 * Open.  Records come in arrival order; lengths[i] is the body length (DTLS
 * 1.3: the fragment length, the datagram's rest minus 16).  Let (M0, bitmap)
 * be the window at the point of the stream where the call's work runs.
 *  1. Parse, per record.  DTLS 1.2: the record fails when its first byte has
 *     (b & 0xe0) == 0x20, its version is not 0xfefd, its epoch is not the
 *     context's, its length field is not explicit + lengths[i] + 16 or exceeds
 *     16704, or lengths[i] > 2^14; types[i] is the header's type byte, s its
 *     48-bit sequence number.  DTLS 1.3: the first byte is 0 0 1 C S L E E; C
 *     must be clear and E E equal epoch & 3 (a context is one epoch: the
 *     caller routes by these bits); S selects a 2- or 1-byte sequence number,
 *     L says whether a length follows, so the header is the first 2 to 5
 *     bytes of the 5-byte slot; a stated length must be lengths[i] + 16;
 *     lengths[i] must be within 1 .. 2^14 + 1.  The mask is computed from the
 *     sample, the sequence bytes are unmasked and s = reconstruct_seqnum(wire,
 *     0xff or 0xffff, M0) (dtls_record.cc:92-120): the value congruent to the
 *     wire bits closest to M0 + 1, the larger one on a tie, within 0 .. 2^48 -
 *     1.  The AD is the received header with the unmasked sequence bytes.
 *     The prefix is not modified.
 *  2. The AEAD opens the parsed records.  DTLS 1.3: the last non-zero byte of
 *     the fragment is types[i] and its index out_lengths[i]; a fragment of
 *     zeros fails.
 *  3. The window, over the records that passed 1 and 2, in index order: record
 *     i fails if ShouldDiscard(s_i) (older than the maximum - 255, or already
 *     seen), else Record(s_i).  Records that failed earlier never touch it.
 * A failed record has status 0, lengths[i] zero bytes of output, out_lengths[i]
 * 0 and in DTLS 1.3 types[i] 0.  record_numbers[i] = epoch << 48 | s for every
 * record that passed step 1, else 0.  DTLS 1.2 writes out_lengths[i] =
 * lengths[i] for an accepted record.  Argument errors as for seal; DTLS 1.3
 * requires out_lengths.
 *
 * One deliberate departure: the reference reconstructs record i against the
 * window's maximum after records 0..i-1, a batch reconstructs every record
 * against M0, so that a forged record cannot disturb its neighbours and step 1
 * stays parallel.  The two agree whenever every genuine record's sequence
 * number s satisfies -step/2 < s - (M0 + 1) <= step/2 with step 65536 (16-bit)
 * or 256 (8-bit sequence numbers): callers whose peer sends 8-bit sequence
 * numbers must keep their batches within that range.  For records in order
 * that is at most 32768 (or 128) records per DTLS 1.3 open call; a longer run
 * is issued as several calls back to back on the stream, each of which sees
 * the window the one before it left.  DTLS 1.2 headers carry all 48 bits and
 * have no such limit.
 *
 * Out of scope: the CBC suites, connection IDs, epoch switching and the
 * derivation of sn_key, the plaintext epoch 0, splitting a datagram into
 * records, padding on DTLS 1.3 seal.  (Many associations in one batch:
 * BSSL_AMD_DTLS_SET below.) */
#define BSSL_AMD_DTLS1_2_VERSION 0xfefd
#define BSSL_AMD_DTLS1_3_VERSION 0xfefc
typedef struct bssl_amd_dtls_aead_st BSSL_AMD_DTLS_AEAD;

/* `aead`: EVP_aead_aes_128_gcm(), EVP_aead_aes_256_gcm() or
 * EVP_aead_chacha20_poly1305().  fixed_iv: 4 bytes for DTLS 1.2 AES-GCM, 12
 * otherwise.  sn_key: DTLS 1.3, the record-number ("sn") key of
 * EVP_AEAD_key_length(aead) bytes; DTLS 1.2: NULL, 0.  seq: the first sequence
 * number of a sealing context (ignored on open).  Checked before any GPU
 * call: a version that is neither DTLS 1.2 nor 1.3, a NULL aead, key or
 * fixed_iv, a sn_key that is missing (DTLS 1.3) or given (DTLS 1.2), a DTLS 1.3
 * epoch of 0 (the plaintext epoch, dtls_record.cc:163-168) or seq > 2^48 - 1 is
 * ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED; the AES-CTR-HMAC and CBC AEADs
 * CIPHER_R_CTRL_NOT_IMPLEMENTED; any other AEAD, or a wrong key_len,
 * fixed_iv_len or sn_key_len, CIPHER_R_UNSUPPORTED_KEY_SIZE. */
BSSL_AMD_EXPORT BSSL_AMD_DTLS_AEAD *BSSL_AMD_DTLS_AEAD_new(
    enum evp_aead_direction_t direction, uint16_t version, const EVP_AEAD *aead,
    const uint8_t *key, size_t key_len, const uint8_t *fixed_iv, size_t fixed_iv_len,
    const uint8_t *sn_key, size_t sn_key_len, uint16_t epoch, uint64_t seq);
/* Waits for the device, zeroes the key material and the window on it. */
BSSL_AMD_EXPORT void BSSL_AMD_DTLS_AEAD_free(BSSL_AMD_DTLS_AEAD *t);
BSSL_AMD_EXPORT size_t BSSL_AMD_DTLS_AEAD_prefix_len(const BSSL_AMD_DTLS_AEAD *t);
/* Seal: the sequence number the next record will use. */
BSSL_AMD_EXPORT uint64_t BSSL_AMD_DTLS_AEAD_sequence(const BSSL_AMD_DTLS_AEAD *t);
/* The read window, HOST memory; both synchronise hip_stream.  bitmap bit k
 * (byte k/8, bit k%8) = sequence number max_seq - k seen.  A new open context
 * has max_seq 0 and an empty bitmap. */
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_AEAD_get_window(BSSL_AMD_DTLS_AEAD *t, uint64_t *max_seq,
                                                  uint8_t bitmap[32], void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_AEAD_set_window(BSSL_AMD_DTLS_AEAD *t, uint64_t max_seq,
                                                  const uint8_t bitmap[32], void *hip_stream);

typedef struct {
  size_t num_records;
  const uint8_t *in; /* device */
  uint8_t *out;      /* device, may equal in */
  const uint64_t *offsets; /* device, or NULL: i * record_stride */
  const uint64_t *lengths; /* device, or NULL: record_len */
  uint64_t record_stride;
  uint64_t record_len;
  uint8_t *types; /* as BSSL_AMD_TLS_RECORDS; may be NULL on open */
  uint8_t type;
  uint8_t *prefix; /* device, prefix_len bytes per record */
  uint8_t *suffix; /* device, the 16-byte tag per record */
  uint8_t *status; /* device, 1 / 0 per record, or NULL */
  uint64_t *out_lengths;    /* device; DTLS 1.3 open: required, else optional */
  uint64_t *record_numbers; /* device, optional: epoch << 48 | sequence of record i */
} BSSL_AMD_DTLS_RECORDS;

BSSL_AMD_EXPORT int BSSL_AMD_DTLS_AEAD_seal_records_device(BSSL_AMD_DTLS_AEAD *t,
                                                           const BSSL_AMD_DTLS_RECORDS *r,
                                                           void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_AEAD_open_records_device(BSSL_AMD_DTLS_AEAD *t,
                                                           const BSSL_AMD_DTLS_RECORDS *r,
                                                           void *hip_stream);

/* ---- DTLS association sets: one record batch across many associations ------
 *
 * BSSL_AMD_DTLS_SET is one direction of up to num_slots slots of ONE version
 * (DTLS 1.2 or 1.3) and ONE AEAD suite.  A slot is what a BSSL_AMD_DTLS_AEAD
 * is -- one direction of one epoch of one association -- with all of its state
 * on the device: key, fixed IV, sn key (DTLS 1.3), epoch, the next write
 * sequence number S[c] (seal), the window's maximum and 256-bit map (open).
 * The caller maps (association, epoch) to slots and routes records by their
 * epoch bits, as for one association.  One call protects a batch that mixes
 * the records of many slots and only enqueues work on hip_stream: seal and
 * open never synchronise it, not for AES-GCM either.  The state of a set lives
 * in stream order: issue all calls of one set on one stream, or order them as
 * if they were.
 *
 * Records [run_start[j], run_start[j+1]) of a batch belong to slot
 * c = run_slot[j]; the record layout is BSSL_AMD_DTLS_RECORDS's.
 *
 * Equivalence.  For a well-formed batch, everything written for the records
 * of run j -- prefix, body, tag, status, types, out_lengths, record_numbers --
 * and the slot's state afterwards are byte for byte what
 * BSSL_AMD_DTLS_AEAD_new(direction, version, aead, key_c, iv_c, sn_c, epoch_c,
 * S[c]), on open with its window set to the slot's, produces for those records
 * in order in one call.  That includes the batch-start reconstruction rule:
 * every DTLS 1.3 record of a run is reconstructed against ITS SLOT's maximum
 * at the point of the stream where the call's work runs, so the 32768 / 128
 * in-order bound holds per slot per call, not per call.
 *
 * Seal.  Record i of run j gets the sequence number S[c] + (i - run_start[j]),
 * and S[c] advances by the run's record count, on the device.  A record whose
 * number would pass 2^48 - 1 fails alone and gets no number, and S[c]
 * saturates at 2^48 (exhausted): the one-association call fails as a whole
 * there, a set does not let one exhausted association fail the others.
 *
 * Open.  The replay windows are per slot: two runs that carry the same
 * sequence numbers are unrelated, a number in one run never moves another
 * run's maximum, and only the records that authenticated touch their slot's
 * window, in index order within their run.
 *
 * Records that fail alone, besides those that fail in the one-association
 * layer -- status 0; body and tag zeroed (a DTLS 1.3 seal: all L + 1 bytes of
 * the fragment); on seal the prefix zeroed; out_lengths[i], types[i] (open)
 * and record_numbers[i] 0; no sequence number consumed and the slot's window
 * untouched by them:
 *   - run_slot[j] is out of range, or the slot is unset or cleared;
 *   - the slot already has an earlier non-empty run in this call: the lowest j
 *     wins, and the slot's counter or window moves by the winning run only.
 *
 * Malformed run_start.  Deliberately stricter than the TLS set: when
 * run_start is not non-decreasing, or run_start[0] != 0, or
 * run_start[num_runs] != num_records, every record of the call fails as above
 * and no slot's sequence number or window changes.  Nothing outside the
 * batch's arrays is read or written.  (The check runs on the device: the call
 * itself still returns 1.)
 *
 * Out of scope: the CBC suites, connection IDs, the plaintext epoch 0, mixed
 * suites or versions in one set, more than one run per slot per call, the
 * derivation of sn keys, splitting a datagram into records. */
typedef struct bssl_amd_dtls_set_st BSSL_AMD_DTLS_SET;

/* The version / aead rules and codes of BSSL_AMD_DTLS_AEAD_new; num_slots 0 or
 * above 2^32 - 2 is ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED.  All checks come before
 * any GPU call.  All slots start unset. */
BSSL_AMD_EXPORT BSSL_AMD_DTLS_SET *BSSL_AMD_DTLS_SET_new(enum evp_aead_direction_t direction,
                                                         uint16_t version, const EVP_AEAD *aead,
                                                         size_t num_slots);
/* Waits for the device, zeroes the key material and the windows on it and
 * frees it. */
BSSL_AMD_EXPORT void BSSL_AMD_DTLS_SET_free(BSSL_AMD_DTLS_SET *s);
BSSL_AMD_EXPORT size_t BSSL_AMD_DTLS_SET_num_slots(const BSSL_AMD_DTLS_SET *s);
/* 13 / 21 / 5, as BSSL_AMD_DTLS_AEAD_prefix_len. */
BSSL_AMD_EXPORT size_t BSSL_AMD_DTLS_SET_prefix_len(const BSSL_AMD_DTLS_SET *s);

/* (Re)key slots first .. first+n-1 from HOST arrays: n keys, n fixed IVs (4
 * bytes each for DTLS 1.2 AES-GCM, 12 otherwise), n sn keys of the key's
 * length (DTLS 1.3; NULL for DTLS 1.2), n epochs, n first write sequence
 * numbers (NULL: all 0; not used by an opening set).  An installed opening
 * slot has an empty window at 0.  Ordered on hip_stream like
 * BSSL_AMD_TLS_SET_set_connections; the host copies of the key material are
 * zeroed before the call returns.  Checked before any GPU call, all
 * ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED: a slot range outside the set, NULL keys,
 * fixed_ivs or epochs, sn_keys missing (DTLS 1.3) or given (DTLS 1.2), a DTLS
 * 1.3 epoch of 0, a sequence number above 2^48 - 1. */
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_SET_set_slots(BSSL_AMD_DTLS_SET *s, size_t first, size_t n,
                                                const uint8_t *keys, const uint8_t *fixed_ivs,
                                                const uint8_t *sn_keys, const uint16_t *epochs,
                                                const uint64_t *seqs, void *hip_stream);
/* Unset slots: key material, counter and window zeroed on the device, in
 * stream order; their records then fail.  Only enqueues work. */
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_SET_clear_slots(BSSL_AMD_DTLS_SET *s, size_t first, size_t n,
                                                  void *hip_stream);
/* A sealing set: the next write sequence numbers of slots first..first+n-1 to
 * HOST memory (0 for an unset slot, 2^48 for an exhausted one); synchronises
 * hip_stream.  An opening set: CIPHER_R_INVALID_OPERATION. */
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_SET_sequences(BSSL_AMD_DTLS_SET *s, size_t first, size_t n,
                                                uint64_t *out, void *hip_stream);
/* An opening set: the read windows of slots first..first+n-1, HOST arrays of n
 * maxima and n 32-byte maps in the bit order of BSSL_AMD_DTLS_AEAD_get_window;
 * both synchronise hip_stream.  With them a live association moves onto the
 * set.  A maximum above 2^48 - 1 is ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED; a
 * sealing set CIPHER_R_INVALID_OPERATION. */
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_SET_get_windows(BSSL_AMD_DTLS_SET *s, size_t first, size_t n,
                                                  uint64_t *max_seqs, uint8_t *bitmaps,
                                                  void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_SET_set_windows(BSSL_AMD_DTLS_SET *s, size_t first, size_t n,
                                                  const uint64_t *max_seqs,
                                                  const uint8_t *bitmaps, void *hip_stream);

typedef struct {
  BSSL_AMD_DTLS_RECORDS records; /* layout exactly as for one association;
                                    at most 2^32 - 2 records */
  size_t num_runs;               /* at most 2^32 - 2 */
  const uint32_t *run_slot;      /* device, num_runs entries */
  const uint64_t *run_start; /* device, num_runs + 1 entries, non-decreasing,
                                run_start[0] = 0, run_start[num_runs] = num_records */
} BSSL_AMD_DTLS_SET_RECORDS;

/* Seal (open) the batch; see above.  Returns 0 with nothing launched and an
 * error queued for argument errors: NULL pointers as for one association,
 * num_runs == 0 with num_records != 0, missing run arrays, a count above
 * 2^32 - 2, DTLS 1.3 open without out_lengths (all
 * ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED), the wrong direction
 * (CIPHER_R_INVALID_OPERATION). */
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_SET_seal_records_device(BSSL_AMD_DTLS_SET *s,
                                                          const BSSL_AMD_DTLS_SET_RECORDS *r,
                                                          void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_DTLS_SET_open_records_device(BSSL_AMD_DTLS_SET *s,
                                                          const BSSL_AMD_DTLS_SET_RECORDS *r,
                                                          void *hip_stream);

/* ---- QUIC packet protection (RFC 9001 5) -----------------------------------
 *
 * BSSL_AMD_QUIC_AEAD is one direction of one key generation of one QUIC
 * connection: the AEAD of RFC 9001 5.3 and the header protection of 5.4 for a
 * batch of packets -- what a QUIC stack otherwise does with one
 * EVP_AEAD_CTX_seal / _open and one AES or ChaCha20 block per packet.  An
 * opening context keeps `expected` -- the largest authenticated packet number
 * + 1, or 0 before any packet -- on the device, so that both calls only enqueue
 * work on hip_stream, for AES-GCM too.  The state of a context lives in stream
 * order: issue all calls of one context on one stream, or order them as if
 * they were.  The AEAD is the plain one, as for DTLS: the context generates its
 * own packet numbers, so its nonces rise strictly by construction.
 *
 * Packets are contiguous, header ++ ciphertext ++ tag in one piece: packet i
 * occupies offsets[i] .. + lengths[i] of `in`, and the same offsets apply to
 * `out`.  O = pn_offsets[i] is the number of header bytes before the
 * packet-number field, N (1..4) the length of that field, pn the packet
 * number:
 *   form    the first byte's top bit: set, a long header, whose first-byte
 *           mask is 0x0f; clear, a short header, mask 0x1f
 *   nonce   iv XOR (0^4 ++ be64(pn))
 *   AD      the unprotected header through the packet-number field, O + N bytes
 *   tag     16 bytes
 *   mask    (RFC 9001 5.4) sample = the 16 bytes at packet offset O + 4 of the
 *           protected packet.  AES suites: the first 5 bytes of AES-ECB(hp_key,
 *           sample); ChaCha20: the first 5 keystream bytes of ChaCha20 with key
 *           hp_key, block counter le32(sample[0..4)), nonce sample[4..16).
 *           byte0 ^= mask[0] & (0x0f or 0x1f); pn byte k ^= mask[1 + k], k < N
 *
 * Seal.  lengths[i] = header + payload; the caller leaves lengths[i] + 16
 * bytes of room in `out`.  The input is the header (O + N bytes, N =
 * pn_lengths[i]) ++ the payload.  Packet i gets pn = next_packet_number() + i
 * and the context advances by n; a packet that fails alone still consumes its
 * number.  The device replaces bits 0..1 of the first byte with N - 1 and the N
 * field bytes with the low N bytes of pn, big-endian, and changes nothing else
 * in the header: the fixed bit, the reserved bits and the key phase are the
 * caller's.  It then seals the payload, writes the tag after it and applies
 * the mask.  A packet fails alone -- status 0, out_lengths[i] 0, all
 * lengths[i] + 16 bytes of its slot in `out` zero -- when N is not in 1..4, O
 * == 0, O + N > lengths[i], or N + the payload length < 4 (the sample would
 * run past the tag; RFC 9001 5.4.2 has the sender pad).  Otherwise
 * out_lengths[i] = lengths[i] + 16.  packet_numbers[i] = pn for every packet.
 * Returns 0 with ERR_R_OVERFLOW and nothing launched when
 * next_packet_number() + n - 1 > 2^62 - 1.
 *
 * Open.  lengths[i] = the whole protected packet.  Let E be `expected` at the
 * point of the stream where the call's work runs.
 *  1. Parse.  The packet fails when O == 0 or lengths[i] < O + 20 (no room for
 *     the sample).  Otherwise the mask is computed from the sample, the first
 *     byte unmasked, N = (byte0 & 3) + 1, N field bytes unmasked and pn =
 *     decode(E, truncated, 8 N) exactly as RFC 9000 A.3: win = 2^(8N), hwin =
 *     win / 2, cand = (E & ~(win - 1)) | truncated; if cand + hwin <= E and
 *     cand < 2^62 - win then cand += win, else if cand > E + hwin and cand >=
 *     win then cand -= win.  A packet that fails here has status 0, its
 *     outputs 0, and nothing of its slot in `out` is written.
 *  2. The AEAD.  The unprotected header, H = O + N bytes, is written to `out`
 *     for every parsed packet whether or not it authenticates: that is how the
 *     caller reads the key-phase and reserved bits.  The AEAD opens the
 *     lengths[i] - H - 16 ciphertext bytes with that header as AD; the
 *     plaintext goes to out + offsets[i] + H.  A packet that does not
 *     authenticate gets that many zero bytes, status 0 and out_lengths[i] 0;
 *     otherwise out_lengths[i] = the payload length.  header_lengths[i] = H
 *     and packet_numbers[i] = pn for every parsed packet.  The last 16 bytes
 *     of the slot in `out` are never written by open.
 *  3. The state.  expected = max(E, 1 + max pn over the packets that
 *     authenticated), on the device.  Packets that failed never move it.
 *
 * One deliberate departure, the DTLS one: every packet of a call is decoded
 * against E, not against the running maximum, so that a forged packet cannot
 * disturb its neighbours and step 1 stays parallel.  A conforming sender's
 * encoding (RFC 9000 17.1) is decodable against any value between its largest
 * acknowledged number and the packet itself, so this holds for conforming
 * peers.  For packets in order the bound per call is 128, 32768, 2^23 or 2^31
 * packets past E for N = 1, 2, 3, 4; a longer run is issued as several calls
 * back to back on the stream, each of which sees the `expected` the one before
 * it left.
 *
 * Argument errors of both calls: a NULL context, packets, or `in` / `out` with
 * packets present, or on seal a uniform pn_length outside 1..4 (pn_lengths
 * NULL), ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED; the wrong direction
 * CIPHER_R_INVALID_OPERATION.  num_packets == 0 returns 1.
 *
 * Out of scope: duplicate detection (RFC 9000 12.3) is the caller's, and
 * packet_numbers serves it; key update -- a context is one key generation, the
 * header-protection key does not change with a key update, so either
 * generation's context unmasks the header and the caller routes by the
 * key-phase bit; Retry and Version Negotiation packets; parsing long headers
 * or coalesced datagrams to find O and the length; AES-128-CCM.  Many
 * connections in one call: BSSL_AMD_QUIC_SET below. */
typedef struct bssl_amd_quic_aead_st BSSL_AMD_QUIC_AEAD;

/* `aead`: EVP_aead_aes_128_gcm(), EVP_aead_aes_256_gcm() or
 * EVP_aead_chacha20_poly1305().  iv: 12 bytes; hp_key: the header-protection
 * key of EVP_AEAD_key_length(aead) bytes.  next_pn: the first packet number of
 * a sealing context (ignored on open, whose `expected` starts at 0).  Checked
 * before any GPU call: a NULL aead, key, iv or hp_key, or next_pn > 2^62 - 1 is
 * ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED; the AES-CTR-HMAC and CBC AEADs
 * CIPHER_R_CTRL_NOT_IMPLEMENTED; any other AEAD, or a wrong key_len, iv_len or
 * hp_key_len, CIPHER_R_UNSUPPORTED_KEY_SIZE. */
BSSL_AMD_EXPORT BSSL_AMD_QUIC_AEAD *BSSL_AMD_QUIC_AEAD_new(
    enum evp_aead_direction_t direction, const EVP_AEAD *aead, const uint8_t *key, size_t key_len,
    const uint8_t *iv, size_t iv_len, const uint8_t *hp_key, size_t hp_key_len, uint64_t next_pn);
/* Waits for the device, zeroes the key material and the state on it. */
BSSL_AMD_EXPORT void BSSL_AMD_QUIC_AEAD_free(BSSL_AMD_QUIC_AEAD *q);
/* Seal: the packet number the next packet will use. */
BSSL_AMD_EXPORT uint64_t BSSL_AMD_QUIC_AEAD_next_packet_number(const BSSL_AMD_QUIC_AEAD *q);
/* `expected` of an opening context (a sealing one: CIPHER_R_INVALID_OPERATION);
 * both synchronise hip_stream.  A value above 2^62 is
 * ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED. */
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_AEAD_get_expected(BSSL_AMD_QUIC_AEAD *q, uint64_t *expected,
                                                    void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_AEAD_set_expected(BSSL_AMD_QUIC_AEAD *q, uint64_t expected,
                                                    void *hip_stream);

typedef struct {
  size_t num_packets;
  const uint8_t *in;       /* device */
  uint8_t *out;            /* device, may equal in */
  const uint64_t *offsets; /* device, or NULL: i * packet_stride */
  const uint64_t *lengths; /* device, or NULL: packet_len */
  uint64_t packet_stride;
  uint64_t packet_len;
  const uint32_t *pn_offsets; /* device, or NULL: pn_offset for every packet */
  uint32_t pn_offset;
  const uint8_t *pn_lengths; /* seal only; device, or NULL: pn_length for every packet */
  uint8_t pn_length;
  uint8_t *status;          /* device, 1 / 0 per packet, or NULL */
  uint64_t *out_lengths;    /* device, optional */
  uint32_t *header_lengths; /* device, optional; open only */
  uint64_t *packet_numbers; /* device, optional */
} BSSL_AMD_QUIC_PACKETS;

BSSL_AMD_EXPORT int BSSL_AMD_QUIC_AEAD_seal_packets_device(BSSL_AMD_QUIC_AEAD *q,
                                                           const BSSL_AMD_QUIC_PACKETS *p,
                                                           void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_AEAD_open_packets_device(BSSL_AMD_QUIC_AEAD *q,
                                                           const BSSL_AMD_QUIC_PACKETS *p,
                                                           void *hip_stream);

/* ---- QUIC connection sets: one packet batch across many connections --------
 *
 * BSSL_AMD_QUIC_SET is one direction of up to num_slots slots of ONE AEAD
 * suite.  A slot is what a BSSL_AMD_QUIC_AEAD is -- one direction of one key
 * generation of one packet-number space of one connection -- with all of its
 * state on the device: the AEAD key, the IV, the expanded header-protection
 * key and one 64-bit number, the next packet number S[c] (seal) or expected[c]
 * (open).  The caller maps (connection, space, key generation) to slots.  One
 * call protects a batch that mixes the packets of many slots and only enqueues
 * work on hip_stream: seal and open never synchronise it, not for AES-GCM
 * either.  The state of a set lives in stream order: issue all calls of one
 * set on one stream, or order them as if they were.
 *
 * Packets [run_start[j], run_start[j+1]) of a batch belong to slot
 * c = run_slot[j]; the packet layout is BSSL_AMD_QUIC_PACKETS's.
 *
 * Equivalence.  For a well-formed batch, everything written for the packets of
 * run j -- the packet's slot in `out`, status, out_lengths, header_lengths,
 * packet_numbers -- and the slot's number afterwards are byte for byte what
 * BSSL_AMD_QUIC_AEAD_new(direction, aead, key_c, iv_c, hp_c, S[c]), on open
 * with `expected` set to the slot's, produces for those packets in order in
 * one call.  That includes the batch-start rule: every packet of a run is
 * decoded against ITS SLOT's `expected` at the point of the stream where the
 * call's work runs, so the 128 / 32768 / 2^23 / 2^31 in-order bound holds per
 * slot per call, not per call.
 *
 * Seal.  Packet k of run j gets pn = S[c] + k, and S[c] advances by the run's
 * packet count, on the device.  A packet that fails in the one-connection
 * layer (N outside 1..4, O == 0, O + N > lengths[i], N + payload < 4) still
 * consumes its number, as it does there.  A packet whose number would pass
 * 2^62 - 1 fails alone as below, and S[c] saturates at 2^62 (exhausted): the
 * one-connection call returns ERR_R_OVERFLOW as a whole there, a set does not
 * let one exhausted connection fail the others.
 *
 * Open.  expected[c] = max(E_c, 1 + max pn over the run's packets that
 * authenticated), on the device.  Packets that fail never move it, and a
 * packet in another run never moves it either, whatever number it decodes to.
 *
 * Packets that fail alone, besides those that fail in the one-connection
 * layer; they consume no number and leave the slot's `expected` untouched:
 *   - run_slot[j] is out of range, or the slot is unset or cleared;
 *   - the slot already has an earlier non-empty run in this call: the lowest j
 *     wins, and the slot moves by the winning run only.
 * On seal such a packet looks like a one-connection failed packet: status 0,
 * out_lengths[i] 0, all lengths[i] + 16 bytes of its slot in `out` zero, and
 * packet_numbers[i] 0.  On open it looks like a one-connection parse failure:
 * status, out_lengths, header_lengths and packet_numbers 0, and nothing of its
 * slot in `out` is written.
 *
 * Malformed run_start.  As for BSSL_AMD_DTLS_SET: when run_start is not
 * non-decreasing, or run_start[0] != 0, or run_start[num_runs] != num_packets,
 * every packet of the call fails as above and no slot changes.  Nothing
 * outside the batch's arrays is read or written, whatever run_start and
 * run_slot hold.  (The check runs on the device: the call itself still
 * returns 1.)
 *
 * Out of scope: key update as an operation -- a new key generation is a fresh
 * slot, installed with the `numbers` the caller's ACK state already knows;
 * duplicate detection; Retry and Version Negotiation packets; mixed suites in
 * one set; more than one run per slot per call; finding O. */
typedef struct bssl_amd_quic_set_st BSSL_AMD_QUIC_SET;

/* The aead rules and codes of BSSL_AMD_QUIC_AEAD_new: a NULL aead, or
 * num_slots 0 or above 2^32 - 2, is ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED; the
 * AES-CTR-HMAC and CBC AEADs CIPHER_R_CTRL_NOT_IMPLEMENTED; any other AEAD than
 * AES-128-GCM, AES-256-GCM or ChaCha20-Poly1305 CIPHER_R_UNSUPPORTED_KEY_SIZE.
 * All checks come before any GPU call.  All slots start unset. */
BSSL_AMD_EXPORT BSSL_AMD_QUIC_SET *BSSL_AMD_QUIC_SET_new(enum evp_aead_direction_t direction,
                                                         const EVP_AEAD *aead, size_t num_slots);
/* Waits for the device, zeroes the key material and the slots on it and frees
 * it. */
BSSL_AMD_EXPORT void BSSL_AMD_QUIC_SET_free(BSSL_AMD_QUIC_SET *s);
BSSL_AMD_EXPORT size_t BSSL_AMD_QUIC_SET_num_slots(const BSSL_AMD_QUIC_SET *s);

/* (Re)key slots first .. first+n-1 from HOST arrays: n keys, n 12-byte IVs, n
 * header-protection keys of the key's length, n numbers (seal: the first
 * packet numbers; open: `expected`; NULL: all 0).  Ordered on hip_stream like
 * BSSL_AMD_DTLS_SET_set_slots, and waits for it: the host copies of the key
 * material are zeroed before the call returns.  Checked before any GPU call,
 * all ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED: a slot range outside the set, NULL
 * keys, ivs or hp_keys, a number above 2^62 - 1 (seal) or above 2^62 (open). */
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_SET_set_slots(BSSL_AMD_QUIC_SET *s, size_t first, size_t n,
                                                const uint8_t *keys, const uint8_t *ivs,
                                                const uint8_t *hp_keys, const uint64_t *numbers,
                                                void *hip_stream);
/* Unset slots: key material and number zeroed on the device, in stream order;
 * their packets then fail.  Only enqueues work. */
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_SET_clear_slots(BSSL_AMD_QUIC_SET *s, size_t first, size_t n,
                                                  void *hip_stream);
/* A sealing set: the next packet numbers of slots first..first+n-1 to HOST
 * memory (0 for an unset slot, 2^62 for an exhausted one); synchronises
 * hip_stream.  An opening set: CIPHER_R_INVALID_OPERATION. */
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_SET_next_packet_numbers(BSSL_AMD_QUIC_SET *s, size_t first,
                                                          size_t n, uint64_t *out,
                                                          void *hip_stream);
/* An opening set: `expected` of slots first..first+n-1, HOST arrays; both
 * synchronise hip_stream.  With them a live connection moves onto the set.  A
 * value above 2^62 is ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED; a sealing set
 * CIPHER_R_INVALID_OPERATION. */
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_SET_get_expected(BSSL_AMD_QUIC_SET *s, size_t first, size_t n,
                                                   uint64_t *out, void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_SET_set_expected(BSSL_AMD_QUIC_SET *s, size_t first, size_t n,
                                                   const uint64_t *expected, void *hip_stream);

typedef struct {
  BSSL_AMD_QUIC_PACKETS packets; /* layout exactly as for one connection;
                                    at most 2^32 - 2 packets */
  size_t num_runs;               /* at most 2^32 - 2 */
  const uint32_t *run_slot;      /* device, num_runs entries */
  const uint64_t *run_start; /* device, num_runs + 1 entries, non-decreasing,
                                run_start[0] = 0, run_start[num_runs] = num_packets */
} BSSL_AMD_QUIC_SET_PACKETS;

/* Seal (open) the batch; see above.  Returns 0 with nothing launched and an
 * error queued for argument errors: a NULL set, packets, or `in` / `out` with
 * packets present, num_runs == 0 with num_packets != 0, missing run arrays, a
 * count above 2^32 - 2, on seal a uniform pn_length outside 1..4 (all
 * ERR_R_SHOULD_NOT_HAVE_BEEN_CALLED), the wrong direction
 * (CIPHER_R_INVALID_OPERATION).  num_packets == 0 returns 1. */
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_SET_seal_packets_device(BSSL_AMD_QUIC_SET *s,
                                                          const BSSL_AMD_QUIC_SET_PACKETS *p,
                                                          void *hip_stream);
BSSL_AMD_EXPORT int BSSL_AMD_QUIC_SET_open_packets_device(BSSL_AMD_QUIC_SET *s,
                                                          const BSSL_AMD_QUIC_SET_PACKETS *p,
                                                          void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* BSSL_AMD_TLS_H */
