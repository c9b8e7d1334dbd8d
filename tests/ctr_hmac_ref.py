"""AES-128/256-CTR-HMAC-SHA256 restated in plain Python: hashlib's SHA-256 and
the CPU oracle's AES block (oracle_aes_encrypt_block through
oracle_lib.aes_block, by ccm_eax_ref._ctr).

TEST INFRASTRUCTURE ONLY: slow and obvious.  The construction
(crypto/cipher/e_aesctrhmac.cc of the reference, restated):

  key        = AES key (16 or 32 bytes) || HMAC key (32 bytes)
  ciphertext = AES-CTR(pt), counter block = nonce (12) || be32(0), be32(1), ...
  tag        = HMAC-SHA256(HMAC key, le64(len(ad)) || le64(len(pt)) || nonce ||
                           ad || zeros to a multiple of 64 || ciphertext)[:tag_len]

It is checked against the reference library's own known answers and sealed
records (tests/test_ctr_hmac_ref.py), which is what lets it check arbitrary
batches.
"""
import hashlib

from ccm_eax_ref import _ctr, derive  # noqa: F401  (derive: the fixtures' input rule)

# name -> (AES key bytes, whole key bytes)
AEADS = {
    "aes-128-ctr-hmac-sha256": (16, 48),
    "aes-256-ctr-hmac-sha256": (32, 64),
}
NONCE_LEN = 12
TAG_LEN = 32
MAX_INPUT = (1 << 36) - 1  # the 32-bit block counter


def _tag(hmac_key, nonce, ad, ct, tag_len):
    hdr = len(ad).to_bytes(8, "little") + len(ct).to_bytes(8, "little") + nonce + ad
    hdr += bytes(-len(hdr) % 64)
    # HMAC (RFC 2104) by hand: the 32-byte key zero-padded to SHA-256's block.
    ipad = bytes(b ^ 0x36 for b in hmac_key + bytes(32))
    opad = bytes(b ^ 0x5c for b in hmac_key + bytes(32))
    inner = hashlib.sha256(ipad + hdr + ct).digest()
    return hashlib.sha256(opad + inner).digest()[:tag_len]


def seal(aead, key, nonce, pt, ad=b"", tag_len=TAG_LEN):
    """(ct, tag), or None where the reference call returns 0."""
    aes_len, key_len = AEADS[aead]
    key, nonce, pt, ad = bytes(key), bytes(nonce), bytes(pt), bytes(ad)
    assert len(key) == key_len and 0 < tag_len <= TAG_LEN
    if len(nonce) != NONCE_LEN or len(pt) > MAX_INPUT:
        return None
    ct = _ctr(key[:aes_len], nonce + bytes(4), pt, 4)
    return ct, _tag(key[aes_len:], nonce, ad, ct, tag_len)


def open_(aead, key, nonce, ct, ad, tag, tag_len=TAG_LEN):
    """The plaintext, or None if the reference call returns 0 (a tag of
    another length than the context's, a wrong nonce length, a mismatch)."""
    aes_len, key_len = AEADS[aead]
    key, nonce, ct, ad, tag = bytes(key), bytes(nonce), bytes(ct), bytes(ad), bytes(tag)
    assert len(key) == key_len
    if len(tag) != tag_len or len(nonce) != NONCE_LEN or len(ct) > MAX_INPUT:
        return None
    if _tag(key[aes_len:], nonce, ad, ct, tag_len) != tag:
        return None
    return _ctr(key[:aes_len], nonce + bytes(4), ct, 4)


def fixture_inputs(rec):
    """(key, nonce, pt, ad) of a ref_ctr_hmac.json record (the rule of
    tests/golden/ref_ctr_hmac_gen.cc: every input is derive(label + "/what"))."""
    label = rec["label"]
    return (derive(label + "/key", AEADS[rec["aead"]][1]), derive(label + "/nonce", NONCE_LEN),
            derive(label + "/pt", rec["pt_len"]), derive(label + "/ad", rec["ad_len"]))
