// internal.h -- definitions shared by the host C-ABI layer and the HIP kernels.
//
// Device data layout (all resident in HBM, 16-byte aligned):
//
//   GcmKeyDev   one per AES-GCM key (12,816 bytes): the AES round keys
//               (T-table and plain forms, and the bitsliced engine's per-round
//               AddRoundKey masks), the GHASH nibble table of H^16 and the
//               powers H^1..H^17 as multipliers of the constant-time VALU
//               product (gf128_ct.h).
//               Equivalent of the reference's GCM128_KEY
//               (crypto/fipsmodule/aes/internal.h:325-334), re-laid-out for the
//               LDS-table GHASH of gcm.hip.
//   ChaChaKeyDev one per ChaCha20-Poly1305 key (32 bytes).
//   CbcKeyDev   one per AES-CCM / AES-EAX key (336 bytes): the plain round
//               keys and EAX's per-key constants (cbcmac.hip).
//   AesHmacKeyDev one per AES-CTR-HMAC-SHA256 or TLS AES-CBC-HMAC key (320
//               bytes): the round keys (TLS: of the context's direction) and
//               HMAC's inner and outer SHA-1 or SHA-256 states (ctr_hmac.hip,
//               tls_cbc.hip).
//   BatchDesc   the record-batch descriptor passed by value to the kernels.
#ifndef BSSL_AMD_INTERNAL_H
#define BSSL_AMD_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>

namespace bssl_amd {

// The scratch block of a batch call, alive in stream order from the call's
// first kernel to its last (scratch.cc): what hipMallocAsync / hipFreeAsync
// promise, without the host wait that HIP's pool adds when it recycles a block
// on a busy stream.  Neither call waits for the stream.
hipError_t scratch_alloc(void **out, size_t bytes, hipStream_t stream);
hipError_t scratch_free(void *ptr, hipStream_t stream);

struct alignas(16) GcmKeyDev {
  // Round keys as little-endian words of the FIPS-197 schedule bytes; the
  // middle rounds (1..nr-1) are stored rotated left by 16 bits, which is how
  // the T-table round of gcm.hip consumes them.
  uint32_t rk[15][4];
  uint32_t nr;
  uint32_t key_bytes;
  uint32_t pad[2];
  // The same schedule unrotated (bitsliced kernel: bit masks per round).
  uint32_t rk_plain[15][4];
  // H^k for k = 1..17 (index 0 unused) in the reversed domain of gf128_ct.h,
  // prepared as multipliers (gf_prep): the constant-time VALU products of the
  // record-end combine, the tag and the AD / J0 hashes (H^17: the one-record
  // kernel folds the tag's last x H into the lane weights).
  uint32_t hpow_ct[18][4];
  // htab16[pos][v] = (element with nibble `pos` equal to v) * H^16, as 4
  // little-endian words of the 16 GCM-order bytes.  Nibble position
  // pos = 2*k + 0 is the high nibble of byte k, 2*k + 1 the low nibble.
  // (Rounds 1-2 also held H, H^2, H^4, H^8, H^32 for the record-end tree,
  // which is now the constant-time VALU product.)
  uint32_t htab16[32][16][4];
  // AddRoundKey of the bitsliced engine (gcm_bs.hip, bs16_aes.h): bsmask[r][i]
  // with i = 32*h + 8*row + bit is the mask XORed into state register (row, h,
  // bit) in round r -- 0xffff in the low half when that bit of round-key
  // column h is set, 0xffff0000 when that bit of column h + 2 is (the engine
  // holds columns h and h + 2 in the two halves of a register).  Read by
  // scalar loads, 64 per round, so no SALU work derives them in the rounds.
  uint32_t bsmask[15][64];
};
static_assert(sizeof(GcmKeyDev) == 240 + 16 + 240 + 18 * 16 + 8192 + 15 * 256, "layout");

struct alignas(16) ChaChaKeyDev {
  uint32_t k[8];
};

// One per AES-CCM / AES-EAX key (336 bytes; cbcmac.hip): the FIPS-197 schedule
// as little-endian words, unrotated, and for EAX the per-key constants of
// aead_aes_eax_init (crypto/cipher/e_aeseax.cc:87-93) B = 2L, P = 4L
// (L = E_K(0^128)) and the OMAC chain values after the tag block,
// E_K(0^15 || t) for t = 0, 1, 2 -- all as little-endian words of their bytes.
// (Not GcmKeyDev: these AEADs read none of its 12.5 KB of GHASH tables.)
struct alignas(16) CbcKeyDev {
  uint32_t rk[15][4];
  uint32_t nr;
  uint32_t pad[3];
  uint32_t eax_b[4];
  uint32_t eax_p[4];
  uint32_t eax_e[3][4];
};
static_assert(sizeof(CbcKeyDev) == 240 + 16 + 32 + 48, "layout");

// One per key of the AEADs that pair AES with HMAC (320 bytes):
// AES-128/256-CTR-HMAC-SHA256 (ctr_hmac.hip; the key is AES key || HMAC key,
// crypto/cipher/e_aesctrhmac.cc:52-109) and TLS AES-CBC-HMAC-SHA1/SHA256
// (tls_cbc.hip; MAC key || AES key, e_tls.cc:75-96).  rk: the FIPS-197
// schedule of the AES key as little-endian words, unrotated -- or, for an
// opening TLS context, the schedule of the equivalent inverse cipher (FIPS-197
// 5.3.5: the round keys in reverse order, InvMixColumns applied to rounds
// 1..nr-1).  inner / outer: HMAC's states after the block (MAC key || zeros)
// XOR 0x36.. / 0x5c.., as FIPS 180-4's words (SHA-1 uses the first five).
struct alignas(16) AesHmacKeyDev {
  uint32_t rk[15][4];
  uint32_t nr;
  uint32_t pad[3];
  uint32_t inner[8];
  uint32_t outer[8];
};
static_assert(sizeof(AesHmacKeyDev) == 240 + 16 + 32 + 32, "layout");

enum AeadKind : int {
  kAeadAesGcm = 0,
  kAeadChaChaPoly = 1,
  kAeadXChaChaPoly = 2,
  kAeadAesGcmSiv = 3,
  kAeadAesCcm = 4,
  kAeadAesEax = 5,
  kAeadAesCtrHmac = 6,
  kAeadTlsCbc = 7
};

// Device chunk descriptors of iovec records: CRYPTO_IOVEC / CRYPTO_IVEC
// (reference include/openssl/aead.h:400-414) on the device.
struct IovecDev {
  uint8_t *out;
  const uint8_t *in;
  uint64_t len;
};
struct IvecDev {
  const uint8_t *in;
  uint64_t len;
};

// Record-batch descriptor (device pointers), see BSSL_AMD_BATCH.
struct BatchDesc {
  const uint8_t *in;
  uint8_t *out;
  const uint64_t *offsets;
  const uint64_t *lengths;
  uint64_t record_stride;
  uint64_t record_len;
  const uint8_t *nonces;
  uint64_t nonce_len;
  const uint8_t *ad;
  const uint64_t *ad_offsets;
  const uint64_t *ad_lengths;
  uint64_t ad_stride;
  uint64_t ad_len;
  uint8_t *tags;
  uint8_t *status;
  const uint32_t *key_index;
  uint64_t num_records;
  uint32_t tag_len;
  uint32_t num_keys;
  // Processing order (device, num_records entries) or null for 0..n-1; set by
  // the launchers for ragged batches (sched.hip), never by callers.
  const uint32_t *order;
  // With `order`: the processing positions one launch covers, [*split_lo,
  // *split_hi) (null: 0 and num_records) -- length classes of a ragged batch
  // (records of 4 KiB or more, the shorter ones, ...), which take kernels with
  // different lanes per record (gcm.hip).
  const uint32_t *split_lo;
  const uint32_t *split_hi;
  // Per-record precondition flags (device, 1 = the record may be sealed) or
  // null: the tls12/tls13 nonce checks of tls_scan.hip.  A record with flag 0
  // fails like a reference call that returned 0 (zeroed output, status 0).
  const uint8_t *valid;
  // Extra trailing message bytes (the reference's `extra_in` of seal_scatter,
  // aead.cc.inc:163-209; the TLS 1.3 inner content type): extra_len bytes per
  // record, read at extra + i*extra_stride and sealed (opened) after the
  // record's `in` bytes; their output goes to extra_out + i*extra_out_stride.
  // Tags are at tags + i*tag_stride (0 = tag_len).  Set by the TLS record
  // layer only; the public batch leaves them 0/null.
  const uint8_t *extra;
  uint8_t *extra_out;
  uint32_t extra_len;
  uint32_t extra_stride;
  uint32_t extra_out_stride;
  uint32_t tag_stride;
  // iovec records walked in place by the AES-GCM kernels (iovec.hip,
  // EVP_AEAD_CTX_sealv_batch_device): when `iovecs` is set, record i's message
  // is the concatenation of iovecs[iovec_start[i] .. iovec_start[i+1]) and its
  // AD that of aadvecs[aadvec_start[i] ..] (or none); `lengths` / `ad_lengths`
  // hold the totals and in / out / offsets / ad are unused.  Null otherwise.
  const IovecDev *iovecs;
  const uint64_t *iovec_start;
  const IvecDev *aadvecs;
  const uint64_t *aadvec_start;
  // Single-record host calls (aead_api.cc one_record): when set, the
  // one-record kernels write done_seq here (mapped host memory) after every
  // other store of the record has completed, so the host can return as soon
  // as it sees the value instead of waiting for the stream.  Null otherwise
  // (the other kernels ignore it).
  uint32_t *done;
  uint32_t done_seq;
  // ... and the record's 12-byte nonce (inl bit 0) and its AD of at most 16
  // bytes, zero-padded (inl bit 1), passed by value, so the one-record kernels
  // start the cipher while the record itself is still in flight.  0 otherwise.
  uint32_t inl;
  uint32_t inl_nonce[3];
  uint32_t inl_ad[4];
  // TLS AES-CBC-HMAC open only (BSSL_AMD_BATCH::out_lengths): record i's
  // plaintext length goes here (0 for a failed record).  Null: not reported.
  uint64_t *out_lengths;
  // TLS AES-CBC-HMAC open only: a record whose plaintext is longer fails like
  // one with a bad MAC (tls_record.cc:204-209, SSL3_RT_MAX_PLAIN_LENGTH).  Set
  // by the TLS record layer only; 0: no limit.
  uint64_t max_plain_len;
  // Set by the QUIC layer only (quic_api.cc): the records of this ragged batch
  // start wherever a header of any length ends, so hardly any is 16-byte
  // aligned.  ChaCha20-Poly1305 then takes its any-alignment kernels, which
  // launch_chacha otherwise picks for unaligned uniform batches only.
  uint32_t any_align;
};

// Tag / extra addresses of record i.
inline __host__ __device__ uint8_t *batch_tag(const BatchDesc &b, uint64_t i) {
  return b.tags + i * (b.tag_stride ? b.tag_stride : b.tag_len);
}
inline __host__ __device__ const uint8_t *batch_extra_in(const BatchDesc &b, uint64_t i) {
  return b.extra + i * b.extra_stride;
}
inline __host__ __device__ uint8_t *batch_extra_out(const BatchDesc &b, uint64_t i) {
  return b.extra_out + i * b.extra_out_stride;
}

// HIP events recorded on the launch stream immediately before and after the
// dominant (bulk) kernel of a batch, for kernel-level timing.
struct KernelEvents {
  void *start;
  void *stop;
};

// Kernel launchers (gcm.hip / chacha.hip).  Return 0 on success or a HIP
// error code.  `ev` (optional) brackets the bulk kernel.
// `engine`: the AES-GCM engine for this batch (GcmEngine; the caller reads
// gcm_engine() once per batch).
int launch_gcm(const GcmKeyDev *keys, const BatchDesc &b, bool open,
               int nr, void *stream, const KernelEvents *ev, int engine);
// AES-GCM engine of the bulk path: the bitsliced table-free engine
// (gcm_bs.hip) or the LDS T-table engine (gcm.hip).  Process-wide; the
// initial value comes from BSSL_AMD_GCM_MODE ("bs" / "bs16" or "table"),
// read once; BSSL_AMD_set_aes_gcm_engine changes it.
enum GcmEngine : int { kGcmEngineTable = 0, kGcmEngineBitsliced = 1, kGcmEngineMix = 2 };
int gcm_engine();
int set_gcm_engine(int engine);  // returns the previous engine, or -1 (bad value)
int launch_gcm_bs(const GcmKeyDev *keys, const BatchDesc &b, bool open, int nr,
                  hipStream_t stream, const KernelEvents *ev);
// The experimental mixed-role engine (gcm_mix.hip; BSSL_AMD_GCM_MODE=mixN,
// N bitsliced waves of 16): eligible batches and the launcher.
int gcm_mix_waves();
int set_gcm_mix(int nb);  // selects the mixed engine with nb bitsliced waves (2, 4, 6)
bool gcm_mix_eligible(const BatchDesc &b, int nr);
int launch_gcm_mix(const GcmKeyDev *keys, const BatchDesc &b, bool open, int nb, hipStream_t s,
                   const KernelEvents *ev);
// Test switch of the table-free engine's batched E_K(J0) production (on by
// default; off: every record end computes its own after the bounded wait).
// Returns the previous setting.
bool set_bs_ek0_producers(bool on);
// Builds `order` (n entries) grouping records by length class, longest first;
// `scratch` holds 128 uint32.  Returns 0 or a HIP error code.
int build_length_order(const uint64_t *lengths, uint64_t n, uint32_t *order, uint32_t *scratch,
                       void *stream);
// The length classes of build_length_order (sched.hip uses these): class
// c = kSchedClasses - 1 - len / kSchedClassBytes (the longest records, of
// (kSchedClasses - 1) * kSchedClassBytes bytes or more, in class 0); scratch
// holds the class histogram, then the class cursors, which end the scatter at
// the end of their class.
constexpr int kSchedClasses = 64;
constexpr uint64_t kSchedClassBytes = 256;
// The scratch word that then holds the number of records of min_len bytes or
// more (a multiple of kSchedClassBytes): the cursor of the last class whose
// records are that long.
constexpr int split_word_for(uint64_t min_len) {
  return kSchedClasses + (kSchedClasses - 1 - (int)(min_len / kSchedClassBytes));
}
// Processing positions [0, scratch[kSplitWord]) hold the records of 4096
// bytes or more, the rest the shorter ones ...
constexpr int kSplitWord = split_word_for(4096);
// ... and [0, scratch[kSplitWord2k]) the records of 2048 bytes or more.
constexpr int kSplitWord2k = split_word_for(2048);
static_assert(kSplitWord == 64 + 47 && kSplitWord2k == 64 + 55, "length classes of sched.hip");
// Whether a batch is worth reordering (ragged and large enough).
inline bool wants_length_order(const BatchDesc &b) {
  return b.lengths && b.num_records >= 4096 && b.num_records < (uint64_t(1) << 32);
}
// AES-GCM-SIV (gcm_siv.hip); uses GcmKeyDev::rk_plain of the master key.
int launch_gcm_siv(const GcmKeyDev *keys, const BatchDesc &b, bool open, int nr, void *stream,
                   const KernelEvents *ev);
// AES-CCM (L = 2; tag_len = M) and AES-EAX (cbcmac.hip), one lane per record.
// BatchDesc::extra and ::iovecs are not supported (error 1); ::done is never
// written.
int launch_cbcmac(const CbcKeyDev *keys, const BatchDesc &b, bool eax, bool open, int nr,
                  void *stream, const KernelEvents *ev);
// AES-128/256-CTR-HMAC-SHA256 (ctr_hmac.hip), one lane per record; tag_len 1
// to 32.  BatchDesc::extra and ::iovecs are not supported (error 1); ::done is
// never written.
int launch_ctr_hmac(const AesHmacKeyDev *keys, const BatchDesc &b, bool open, int nr, void *stream,
                    const KernelEvents *ev);
// The TLS AES-CBC-HMAC AEADs (tls_cbc.hip), one lane per record.  sha1: the
// MAC is HMAC-SHA1 (20 bytes), else HMAC-SHA256 (32); tag_len is the tag slot
// stride (the AEAD's overhead, 36 or 48).  Seal: `keys` hold encryption
// schedules, the tag (MAC and padding, ciphertext) goes to the record's slot.
// Open: `keys` hold equivalent-inverse schedules, the records are whole wire
// fragments, `tags` is unused.  BatchDesc::extra and ::iovecs are not
// supported (error 1); ::done is never written.
int launch_tls_cbc(const AesHmacKeyDev *keys, const BatchDesc &b, bool sha1, bool open, int nr,
                   void *stream, const KernelEvents *ev);
// Its message limit: the 32-bit block counter (e_aesctrhmac.cc:190, 226).
constexpr uint64_t kCtrHmacMaxInput = (uint64_t(1) << 36) - 1;
// CCM's message limit with L = 2 (CRYPTO_ccm128_max_input).
constexpr uint64_t kCcmMaxInput = 65535;
// xchacha: XChaCha20-Poly1305 (24-byte nonces, per-record HChaCha20 subkey).
int launch_chacha(const ChaChaKeyDev *keys, const BatchDesc &b, bool open, bool xchacha,
                  void *stream, const KernelEvents *ev);
// Whether launch_gcm / launch_chacha would run this batch on a one-record
// kernel, the only kernels that write the completion word BatchDesc::done.
bool gcm_takes_one_record_kernel(const BatchDesc &b, int engine);
bool chacha_takes_one_record_kernel(const BatchDesc &b);
// tls12 / tls13 nonce checks over a batch of seal calls (tls_scan.hip):
// writes valid[i] (device) and advances the context's nonce state in place
// (min_next_nonce, mask); synchronises `stream`.  and_into: valid[i] &= the
// check instead of =.  Returns 0 or an error code.
int tls_nonce_scan(const uint8_t *nonces, uint64_t n, int tls, uint64_t *min_next,
                   uint64_t *mask, uint8_t *valid, int and_into, void *stream);
// TLS record layer (tls_records.hip): per-record nonce, header/prefix, AD and
// inner type of a batch of records with sequence numbers seq .. seq + n - 1.
struct TlsPrepare {
  uint64_t n;
  const uint64_t *lengths;  // or record_len for all
  uint64_t record_len;
  const uint8_t *types;     // or `type` for all
  uint8_t type;
  uint8_t fixed_iv[12];
  uint64_t seq;
  int xor_nonce;            // fixed_iv XOR seq (TLS 1.3, TLS 1.2 ChaCha) vs fixed || seq
  int tls13;
  uint16_t record_version;  // header and TLS 1.2 AD version (0x0303)
  uint32_t explicit_len;    // 8 for TLS 1.2 AES-GCM, else 0
  uint32_t extra_len;       // 1 for TLS 1.3 (inner type), else 0
  uint32_t tag_len;
  uint32_t prefix_len;      // 5 + explicit_len
  uint32_t ad_stride;       // 13 (TLS 1.2) or 5 (TLS 1.3)
  int open;                 // records are received: header/explicit nonce read from prefix
  uint8_t *nonces, *prefix, *ad, *extra, *valid;
  // The TLS 1.3 padded form (tls_pad.hip): `lengths` are fragment lengths F,
  // extra_len is 0.  Seal: valid[i] is the pre-pass's and is left alone.
  // Open: the received header's checks go into valid[i].
  int padded;
  // Padded seal in a set: the caller's out_lengths (or null), zeroed for a
  // record that gets no sequence number.
  uint64_t *out_lengths;
};
int launch_tls_prepare(const TlsPrepare &p, void *stream);
// TLS 1.3 record padding (tls_pad.hip).  The seal pre-pass: from record i's
// content length, type and padding (pad_lengths[i], or up to a multiple of
// pad_block; 0 or 1: none) the fragment length -- frag_len[i] = F, valid[i] =
// 1, out_lengths[i] = F (when given), the content copied when out != in, then
// the type byte and the zeros; or for a record that cannot be sealed
// frag_len[i] = the content length, valid[i] = 0, out_lengths[i] = 0.
struct TlsPadSeal {
  uint64_t n;
  const uint8_t *in;
  uint8_t *out;
  const uint64_t *offsets;  // or i * record_stride
  const uint64_t *lengths;  // or record_len for all
  uint64_t record_stride;
  uint64_t record_len;
  const uint8_t *types;     // or `type` for all
  uint8_t type;
  const uint32_t *pad_lengths;
  uint32_t pad_block;
  uint64_t *frag_len;
  uint64_t *out_lengths;
  uint8_t *valid;
};
int launch_tls13_pad_seal(const TlsPadSeal &p, void *stream);
// The open post-pass: for every record with status[i] != 0 the last non-zero
// byte of the opened fragment goes to types[i] and its index to
// out_lengths[i]; a fragment of zeros gets status[i] = 0.  Every other record:
// types[i] = 0, out_lengths[i] = 0.  No pointer may be null but offsets and
// lengths.
struct TlsPadStrip {
  uint64_t n;
  const uint8_t *out;
  const uint64_t *offsets;
  const uint64_t *lengths;  // fragment lengths
  uint64_t record_stride;
  uint64_t record_len;
  uint8_t *status;
  uint8_t *types;
  uint64_t *out_lengths;
};
int launch_tls13_pad_strip(const TlsPadStrip &p, void *stream);
// TLS connection sets (tls_set.hip; BSSL_AMD_TLS_SET): the per-connection
// record-layer state on the device, one entry per slot.  All zero: unset.
struct alignas(16) TlsSetConn {
  uint64_t seq;     // the connection's next sequence number
  // The fixed IV (TLS 1.2 AES-GCM: 4 bytes, then zeros): bytes 0..7 and
  // 8..11, little-endian (TlsIv, tls_prepare.h).
  uint64_t iv_lo;
  uint32_t iv_hi;
  uint32_t live;    // 1: keys and IV installed
  // Within one call: ~j of the lowest non-empty run j that names this
  // connection (atomicMax; 0: none).  0 between calls.
  uint32_t claim;
  uint32_t pad;
};
static_assert(sizeof(TlsSetConn) == 32, "layout");
// The runs of a batch over a set (set_runs.h): records [run_start[j],
// run_start[j+1]) belong to slot run_slot[j] of num_slots; key_index[i] is
// written with record i's slot (0 for a record that has none).  Scratch of the
// DTLS and QUIC sets alone (the TLS set has none of it and leaves them null):
//   flag      one word, zero: set when run_start is malformed
//   run_of    per record: j + 1 of the run whose slot the record was prepared
//             with, 0 for a record that has none
//   run_won   per run: c + 1 when run j won the live slot c in a well-formed
//             batch, else 0 (the advance kernel, for the steps that follow)
struct SetRuns {
  uint32_t num_slots;
  uint64_t num_runs;
  const uint32_t *run_slot;
  const uint64_t *run_start;  // num_runs + 1 entries
  uint32_t *key_index;
  uint32_t *flag;
  uint32_t *run_of;
  uint32_t *run_won;
};
// A batch of records of many connections.  rec.fixed_iv and rec.seq are unused
// (they come from conns[c]); rec.valid and runs.key_index are written for every
// record.
struct TlsSetPrepare {
  TlsPrepare rec;
  TlsSetConn *conns;
  SetRuns runs;
};
// Three launches in stream order: the runs claim their connections, every
// record is prepared with its connection's next sequence number (or failed),
// the runs that won advance their connections.  0 or a HIP error code.
int launch_tls_set_prepare(const TlsSetPrepare &p, void *stream);
// ... and of the TLS 1.1 / 1.2 AES-CBC-HMAC suites: the 16-byte CBC IV (seal:
// the caller's, or bytes 0..15 of the ChaCha20 block of iv_key with counter
// (uint32)seq and nonce words (uint32)(seq >> 32), 0, 0; open: the received
// one, prefix + 5), the 11-byte AD be64(seq) || type || version, on seal the
// 21-byte prefix (header with the padded length, then the IV), on open the
// header type; and valid[i] = 0 for the publicly invalid records.
struct TlsCbcPrepare {
  uint64_t n;
  const uint64_t *lengths;  // or record_len for all
  uint64_t record_len;
  const uint8_t *types;     // seal: or `type` for all
  uint8_t type;
  uint16_t record_version;  // 0x0302 or 0x0303: header and AD
  uint32_t mac_len;         // 20 or 32
  uint64_t seq;
  int open;
  const uint8_t *explicit_ivs;  // seal: 16 bytes per record, or null: generated
  uint32_t iv_key[8];           // the generator's key, little-endian words
  uint8_t *nonces, *prefix, *ad, *valid;
  uint8_t *types_out;           // open: receives the header types, or null
};
int launch_tls_cbc_prepare(const TlsCbcPrepare &p, void *stream);
// DTLS record protection (dtls.hip, dtls_prepare.h; BSSL_AMD_DTLS_AEAD): what
// one direction of one epoch keeps on the device.
struct alignas(16) DtlsState {
  // The read window (DTLSReplayBitmap, dtls_record.cc:29-57): bit k of the
  // 256-bit map (word k / 64, bit k % 64) = sequence number max_seq - k seen.
  uint64_t max_seq;
  uint64_t bitmap[4];
  uint64_t pad;
  // DTLS 1.3: the record-number key -- the FIPS-197 schedule as little-endian
  // words, unrotated (AES suites), or the ChaCha20 key's eight words in
  // sn[0..7].
  uint32_t sn[60];
  uint32_t pad2[4];
};
static_assert(sizeof(DtlsState) == 48 + 256, "layout");
// How a DTLS 1.3 context computes the record-number mask (RFC 9147 4.2.3).
enum DtlsMask : int { kDtlsMaskNone = 0, kDtlsMaskAes128 = 1, kDtlsMaskAes256 = 2, kDtlsMaskChaCha = 3 };
constexpr uint64_t kDtlsMaxSequence = (uint64_t(1) << 48) - 1;
// Step 1 of a batch (dtls_prepare_kernel), one lane per record.  Seal: the
// header (and DTLS 1.2 AES-GCM's explicit nonce) into the prefix, zeros for a
// record that fails; nonce and AD into the scratch; record_numbers[i].  Open:
// the received header's checks into valid[i], the header type (DTLS 1.2), the
// sequence number (DTLS 1.3: unmasked and reconstructed against the window's
// maximum), nonce, AD and its length, seqs[i] and record_numbers[i].
struct DtlsPrepare {
  uint64_t n;
  const uint8_t *body;      // open, DTLS 1.3: the fragments (the mask's sample)
  const uint64_t *offsets;  // or i * record_stride
  const uint64_t *lengths;  // or record_len for all; DTLS 1.3: fragment lengths
  uint64_t record_stride;
  uint64_t record_len;
  const uint8_t *types;     // seal, DTLS 1.2: or `type` for all
  uint8_t type;
  uint8_t *types_out;       // open, DTLS 1.2: receives the header types, or null
  uint8_t fixed_iv[12];
  uint16_t epoch;
  uint64_t seq;             // seal: the first record's sequence number
  int open;
  int dtls13;
  int xor_nonce;            // fixed_iv XOR sequence vs the 4-byte IV || explicit nonce
  uint32_t prefix_len;      // 13, 21 or 5
  uint32_t ad_stride;       // 13 or 5
  uint8_t *prefix;
  const uint8_t *suffix;    // the tags (open, DTLS 1.3: the sample's continuation)
  uint8_t *nonces, *ad, *valid;
  uint64_t *ad_lengths;     // open, DTLS 1.3: 2 to 5
  uint64_t *seqs;           // open: the records' sequence numbers, for the window
  uint64_t *record_numbers; // or null
  uint64_t *out_lengths;    // seal, DTLS 1.2: the body length or 0 (failed); or null
  const DtlsState *state;
};
int launch_dtls_prepare(const DtlsPrepare &p, int mask, void *stream);
// After a DTLS 1.3 seal: header bytes 1..2 of every record with status[i] != 0
// XOR the first two mask bytes; the sample is the first 16 bytes of fragment ||
// tag.
struct DtlsMaskSeal {
  uint64_t n;
  const uint8_t *body;
  const uint64_t *offsets;
  const uint64_t *lengths;  // fragment lengths
  uint64_t record_stride;
  uint64_t record_len;
  uint8_t *prefix;          // 5 bytes per record
  const uint8_t *suffix;    // 16 bytes per record
  const uint8_t *status;
  const DtlsState *state;
};
int launch_dtls_mask(const DtlsMaskSeal &p, int mask, void *stream);
// Step 3 of an open: the replay window over the records with status[i] != 0,
// in index order, as three launches (dtls.hip).  A record the window refuses
// gets status 0, lengths[i] zero bytes of output, out_lengths[i] 0 and (DTLS
// 1.3) types[i] 0.  table: 2 * table_slots uint64 (all ones), block_max: one
// uint64 per 256 records, old: 5 uint64 -- scratch.
struct DtlsWindow {
  uint64_t n;
  uint8_t *out;
  const uint64_t *offsets;
  const uint64_t *lengths;
  uint64_t record_stride;
  uint64_t record_len;
  uint8_t *status;
  uint64_t *out_lengths;  // or null
  int set_lengths;        // DTLS 1.2: out_lengths[i] = lengths[i] for an accepted record
  uint8_t *types;         // DTLS 1.3, or null
  const uint64_t *seqs;
  uint64_t *table;
  uint64_t table_slots;   // a power of two, at least 2 n
  uint64_t *block_max;
  uint64_t *old;
  DtlsState *state;
};
int launch_dtls_window(const DtlsWindow &p, void *stream);
// DTLS association sets (dtls_set.hip; BSSL_AMD_DTLS_SET): what a slot -- one
// direction of one epoch of one association -- keeps on the device.  All zero:
// unset.
struct alignas(16) DtlsSetSlot {
  // Seal: the next write sequence number; 2^48: exhausted.
  uint64_t seq;
  // Open: the read window, as DtlsState has it.
  uint64_t max_seq;
  uint64_t bitmap[4];
  // The fixed IV as TlsSetConn has it (DTLS 1.2 AES-GCM: 4 bytes, then zeros).
  uint64_t iv_lo;
  uint32_t iv_hi;
  uint32_t live;   // 1: keys, IV and epoch installed
  // Within one call: ~j of the lowest non-empty run j that names this slot
  // (atomicMax; 0: none).  0 between calls.
  uint32_t claim;
  uint32_t epoch;
  uint64_t pad;
  // DTLS 1.3: the record-number key, as DtlsState::sn.
  uint32_t sn[60];
};
static_assert(sizeof(DtlsSetSlot) == 80 + 240, "layout");
// One batch over many slots.  rec.fixed_iv, rec.epoch, rec.seq and rec.state
// are unused (they come from the slot); rec.valid, rec.seqs (open) and
// runs.key_index are written for every record.
struct DtlsSetPrepare {
  DtlsPrepare rec;
  DtlsSetSlot *slots;
  SetRuns runs;
};
// Three launches in stream order: the runs claim their slots and check
// run_start, every record is prepared from its slot (or failed), the runs that
// won advance their slots' write sequence numbers (seal) and clear the claims.
int launch_dtls_set_prepare(const DtlsSetPrepare &p, int mask, void *stream);
// After a DTLS 1.3 seal: DtlsMaskSeal with record i's key in slots[key_index[i]]
// (m.state is unused).
int launch_dtls_set_mask(const DtlsMaskSeal &m, const DtlsSetSlot *slots, uint32_t num_slots,
                         const uint32_t *key_index, int mask, void *stream);
// Step 3 of an open over a set: one window per slot, over each run's records
// with status[i] != 0 in index order (w.state, w.old and w.block_max are
// unused; w.table holds table_slots uint32 record indices, all ones).  run_max:
// one zeroed uint64 per run; old: 6 uint64 per run; block_r / block_s: one
// entry per 256 records.
struct DtlsSetWindow {
  DtlsWindow w;
  DtlsSetSlot *slots;
  uint64_t num_runs;
  const uint32_t *run_of;
  const uint32_t *run_won;
  uint64_t *run_max;
  uint64_t *old;
  uint32_t *block_r;
  uint64_t *block_s;
};
int launch_dtls_set_window(const DtlsSetWindow &p, void *stream);
// QUIC packet protection (quic.hip, quic_prepare.h; BSSL_AMD_QUIC_AEAD): what
// one direction of one key generation of a connection keeps on the device.
struct alignas(16) QuicState {
  // Open: the largest authenticated packet number + 1, 0 before any packet.
  uint64_t expected;
  uint64_t pad;
  // The header-protection key, as DtlsState::sn.
  uint32_t hp[60];
  uint32_t pad2[4];
};
static_assert(sizeof(QuicState) == 16 + 256, "layout");
constexpr uint64_t kQuicMaxPacketNumber = (uint64_t(1) << 62) - 1;
// Step 1 of a batch (quic_prepare_kernel), one lane per packet.  Seal: the
// header into `out` with the packet-number length bits and field of pn =
// next_pn + i.  Open: the mask from the sample, the unmasked header into `out`,
// the decoded packet number, the tag into tags + 16 i.  Both: the nonce, the
// body's offset and length and the header length for the bulk kernels (a packet
// that fails here: length 0, valid 0).
struct QuicPrepare {
  uint64_t n;
  const uint8_t *in;
  uint8_t *out;
  const uint64_t *offsets;     // or i * packet_stride
  const uint64_t *lengths;     // or packet_len for all
  uint64_t packet_stride;
  uint64_t packet_len;
  const uint32_t *pn_offsets;  // or pn_offset for all
  uint32_t pn_offset;
  const uint8_t *pn_lengths;   // seal: or pn_length for all
  uint8_t pn_length;
  uint8_t iv[12];
  uint64_t next_pn;            // seal
  int open;
  uint8_t *nonces, *valid;
  uint8_t *tags;               // open: 16 bytes per packet
  uint64_t *body_offsets, *body_lengths, *ad_lengths;
  uint64_t *pns;               // open: the decoded numbers, for the state step
  uint32_t *header_lengths;    // open, or null
  uint64_t *packet_numbers;    // or null
  const QuicState *state;
};
int launch_quic_prepare(const QuicPrepare &p, int mask, void *stream);
// After a seal: the tag from tags + 16 i to the packet's end, the 5-byte mask
// of the sample onto the first byte and the packet-number field of every
// packet with status[i] != 0; the whole slot of a failed one zeroed.
struct QuicProtect {
  uint64_t n;
  uint8_t *out;
  const uint64_t *offsets;
  const uint64_t *lengths;
  uint64_t packet_stride;
  uint64_t packet_len;
  const uint64_t *body_offsets, *body_lengths;
  const uint8_t *tags;
  const uint8_t *status;
  uint64_t *out_lengths;  // or null
  const QuicState *state;
};
int launch_quic_protect(const QuicProtect &p, int mask, void *stream);
// Step 3 of an open: out_lengths[i], and expected = max(expected, 1 + pns[i])
// over the packets with status[i] != 0.
struct QuicExpected {
  uint64_t n;
  const uint8_t *status;
  const uint64_t *pns, *body_lengths;
  uint64_t *out_lengths;  // or null
  QuicState *state;
};
int launch_quic_expected(const QuicExpected &p, void *stream);
// QUIC connection sets (quic_set.hip; BSSL_AMD_QUIC_SET): what a slot -- one
// direction of one key generation of one packet-number space of one connection
// -- keeps on the device.  All zero: unset.
struct alignas(16) QuicSetSlot {
  // Seal: the next packet number S, 2^62: exhausted.  Open: `expected`.
  uint64_t pn;
  // The IV as TlsSetConn has it.
  uint64_t iv_lo;
  uint32_t iv_hi;
  uint32_t live;   // 1: keys and IV installed
  // Within one call: ~j of the lowest non-empty run j that names this slot
  // (atomicMax; 0: none).  0 between calls.
  uint32_t claim;
  uint32_t pad;
  // The header-protection key, as QuicState::hp.
  uint32_t hp[60];
};
static_assert(sizeof(QuicSetSlot) == 32 + 240, "layout");
// One batch over many slots.  pk.iv, pk.next_pn and pk.state are unused (they
// come from the slot); pk.valid, pk.pns (open) and runs.key_index are written
// for every packet.
struct QuicSetPrepare {
  QuicPrepare pk;
  QuicSetSlot *slots;
  SetRuns runs;
};
// Three launches in stream order: the runs claim their slots and check
// run_start, every packet is prepared from its slot (or failed), the runs that
// won advance their slots' packet numbers (seal) and clear the claims.
int launch_quic_set_prepare(const QuicSetPrepare &p, int mask, void *stream);
// After a seal: QuicProtect with packet i's header-protection key in
// slots[key_index[i]] (m.state is unused).
int launch_quic_set_protect(const QuicProtect &m, const QuicSetSlot *slots, uint32_t num_slots,
                            const uint32_t *key_index, int mask, void *stream);
// Step 3 of an open over a set: out_lengths[i], and for every run that won its
// slot, the slot's expected = max(expected, 1 + pns[i]) over the run's packets
// with status[i] != 0 (e.state is unused).
struct QuicSetExpected {
  QuicExpected e;
  QuicSetSlot *slots;
  uint32_t num_slots;
  uint64_t num_runs;
  const uint32_t *run_of;
  const uint32_t *run_won;
};
int launch_quic_set_expected(const QuicSetExpected &p, void *stream);
// Record-layer limits (include/openssl/ssl3.h of the reference).
constexpr uint64_t kTlsMaxPlainLen = 16384;
constexpr uint64_t kTlsMaxEncryptedLen = 16384 + 320;
// Batches of non-contiguous records (iovec.hip).
struct IovBatchDesc {
  uint64_t num_records;
  const IovecDev *iovecs;
  const uint64_t *iovec_start;   // num_records + 1 entries
  const IvecDev *aadvecs;        // or null (no AD)
  const uint64_t *aadvec_start;  // num_records + 1 entries
  const uint8_t *nonces;
  uint64_t nonce_len;
  uint8_t *tags;
  uint8_t *status;
};
// Runs the bulk kernels over an iovec batch (a BatchDesc with `iovecs` set,
// whose tag_len / key fields the runner fills in).  Returns 0 or an error.
struct IovRunner {
  virtual int operator()(BatchDesc &d) const = 0;
};
// Per-record totals -> run; no staging, no stream synchronisation.
int iov_batch_run(const IovBatchDesc &b, const IovRunner &run, void *stream);
int launch_synth(uint64_t first, size_t n, const uint64_t *offsets,
                 const uint64_t *lengths, uint8_t *pt, uint8_t *nonces,
                 uint8_t *ads, void *stream);

// Compute units of the current device, cached per device ordinal (launch
// grids of the persistent kernels; 0 on error).
inline int device_cu_count() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
  if (dev < 64) {
    const int v = cache[dev].load(std::memory_order_relaxed);
    if (v) return v;
  }
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  if (dev < 64) cache[dev].store(v, std::memory_order_relaxed);
  return v;
}

// Wipes key material that goes out of scope (reference: OPENSSL_cleanse).
void secure_zero(void *p, size_t n);

// Key setup (key_setup.cc, key_sched.h): one key on the host, or n keys by
// the device kernel into device memory (synchronous on `s`; 0 or an error).
bool gcm_key_setup(const uint8_t *key, size_t key_len, GcmKeyDev *out);
int gcm_key_setup_device(const uint8_t *keys, size_t key_len, size_t n, GcmKeyDev *out,
                         hipStream_t s);
void chacha_key_setup(const uint8_t *key, ChaChaKeyDev *out);
// AES-CCM / AES-EAX key (host only); false for a bad key length.
bool cbc_key_setup(const uint8_t *key, size_t key_len, CbcKeyDev *out);
// A record-number or header-protection key (DtlsMask `mask`) ORed into the
// zeroed words of DtlsState::sn and its like: the AES schedule, or ChaCha20's
// eight key words; nothing for kDtlsMaskNone.  false for a bad key length.
bool mask_key_words(int mask, const uint8_t *key, size_t key_len, uint32_t out[60]);
// AES-CTR-HMAC-SHA256 key, AES key || 32-byte HMAC key (host only); false for
// a bad key length.
bool ctr_hmac_key_setup(const uint8_t *key, size_t key_len, AesHmacKeyDev *out);
// TLS AES-CBC-HMAC key, MAC key (mac_len: 20 or 32 bytes) || AES key (host
// only); open: the schedule of the equivalent inverse cipher.  false for a bad
// key length.
bool tls_cbc_key_setup(const uint8_t *key, size_t key_len, size_t mac_len, bool open,
                       AesHmacKeyDev *out);
// Key counts from which make_keys builds AES-GCM tables on the device.
constexpr size_t kDeviceKeySetupMin = 64;

}  // namespace bssl_amd

#endif
