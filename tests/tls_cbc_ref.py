"""The TLS AES-CBC-HMAC AEADs (explicit IV) restated in plain Python: hashlib's
SHA-1 / SHA-256 with HMAC by hand, the CPU oracle's AES block for encryption
(oracle_lib.aes_block) and a byte-wise FIPS-197 inverse cipher written out
here (the oracle has no decryption).

TEST INFRASTRUCTURE ONLY: slow and obvious.  The construction
(crypto/cipher/e_tls.cc and tls_cbc.cc of the reference, restated):

  key  = MAC key (20 bytes SHA-1, 32 bytes SHA-256) || AES key (16 or 32)
  mac  = HMAC(MAC key, ad (11 bytes) || be16(len(pt) mod 2^16) || pt)
  wire = AES-CBC(iv = nonce, pt || mac || pad_len x byte(pad_len - 1)),
         pad_len = 16 - (len(pt) + mac_len) % 16 on seal; open accepts any
         padding of 1..256 bytes whose bytes all equal pad_len - 1
  seal returns wire[:len(pt)] and the "tag" wire[len(pt):]

It is checked against the reference library's own known answers and sealed
records (tests/test_tls_cbc_ref.py), which is what lets it check arbitrary
batches.
"""
import functools
import hashlib
import json
import lzma
import os

import oracle_lib as o
from ccm_eax_ref import derive  # noqa: F401  (the fixtures' input rule)

# name -> (hash name, MAC bytes, AES key bytes)
AEADS = {
    "aes-128-cbc-sha1-tls": ("sha1", 20, 16),
    "aes-256-cbc-sha1-tls": ("sha1", 20, 32),
    "aes-128-cbc-sha256-tls": ("sha256", 32, 16),
}
NONCE_LEN = 16
AD_LEN = 11


def key_len(aead):
    return AEADS[aead][1] + AEADS[aead][2]


def mac_len(aead):
    return AEADS[aead][1]


def overhead(aead):
    return AEADS[aead][1] + 16


def tag_len(aead, pt_len):
    """EVP_AEAD_CTX_tag_len: the MAC and the minimal padding."""
    m = AEADS[aead][1]
    return m + 16 - (pt_len + m) % 16


# ---- FIPS-197 inverse cipher, byte-wise ---------------------------------------

def _xtime(a):
    return ((a << 1) ^ 0x1b) & 0xff if a & 0x80 else a << 1


def _mul(a, b):
    p = 0
    while b:
        if b & 1:
            p ^= a
        a = _xtime(a)
        b >>= 1
    return p


def _make_sbox():
    # 5.1.1: the multiplicative inverse (x^254), then the affine map.
    sbox = []
    for x in range(256):
        inv, base, e = 1, x, 254
        while e:
            if e & 1:
                inv = _mul(inv, base)
            base = _mul(base, base)
            e >>= 1
        if x == 0:
            inv = 0
        s = inv
        for i in range(1, 5):
            s ^= ((inv << i) | (inv >> (8 - i))) & 0xff
        sbox.append(s ^ 0x63)
    return sbox


SBOX = _make_sbox()
INV_SBOX = [0] * 256
for _i, _s in enumerate(SBOX):
    INV_SBOX[_s] = _i


# InvMixColumns' multiples, tabulated (the byte-wise products, computed once).
_M9, _M11, _M13, _M14 = ([_mul(x, k) for x in range(256)] for k in (0x09, 0x0b, 0x0d, 0x0e))


@functools.lru_cache(maxsize=1024)
def key_expansion(key):
    """5.2: the round keys as a list of 16-byte blocks."""
    nk = len(key) // 4
    nr = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        elif nk > 6 and i % nk == 4:
            t = [SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return [bytes(sum(w[4 * r:4 * r + 4], [])) for r in range(nr + 1)]


def aes_decrypt_block(key, block):
    """5.3 InvCipher: state byte r + 4c is row r of column c."""
    rks = key_expansion(bytes(key))
    nr = len(rks) - 1
    s = [a ^ b for a, b in zip(block, rks[nr])]
    for rnd in range(nr - 1, -1, -1):
        # InvShiftRows: row r moves right by r columns
        s = [s[r + 4 * ((c - r) % 4)] for c in range(4) for r in range(4)]
        s = [INV_SBOX[b] for b in s]
        s = [a ^ b for a, b in zip(s, rks[rnd])]
        if rnd:
            t = []
            for c in range(4):
                col = s[4 * c:4 * c + 4]
                for r in range(4):
                    t.append(_M14[col[r]] ^ _M11[col[(r + 1) % 4]] ^
                             _M13[col[(r + 2) % 4]] ^ _M9[col[(r + 3) % 4]])
            s = t
    return bytes(s)


# ---- the construction ----------------------------------------------------------

def _hmac(hash_name, mac_key, msg):
    # RFC 2104 by hand: the key zero-padded to the 64-byte block of both hashes.
    k = mac_key + bytes(64 - len(mac_key))
    inner = hashlib.new(hash_name, bytes(b ^ 0x36 for b in k) + msg).digest()
    return hashlib.new(hash_name, bytes(b ^ 0x5c for b in k) + inner).digest()


def _mac(aead, key, ad, data):
    h, m, _ = AEADS[aead]
    return _hmac(h, key[:m], ad + (len(data) & 0xffff).to_bytes(2, "big") + data)


def seal(aead, key, nonce, pt, ad, pad_len=None):
    """The wire fragment (the first len(pt) bytes are the ciphertext body, the
    rest the tag), or None where the reference call returns 0.  pad_len: a
    padding length of the caller's choice (1..256, making the total a multiple
    of 16), for feeding open non-minimal padding; default: minimal."""
    key, nonce, pt, ad = bytes(key), bytes(nonce), bytes(pt), bytes(ad)
    assert len(key) == key_len(aead)
    if len(nonce) != NONCE_LEN or len(ad) != AD_LEN:
        return None
    return cbc_encrypt(key[mac_len(aead):], nonce, plain_of(aead, key, pt, ad, pad_len))


def plain_of(aead, key, pt, ad, pad_len=None):
    """What CBC encrypts, and what a successful open leaves in `out`:
    pt || mac || padding."""
    m = mac_len(aead)
    if pad_len is None:
        pad_len = 16 - (len(pt) + m) % 16
    assert 1 <= pad_len <= 256 and (len(pt) + m + pad_len) % 16 == 0
    return bytes(pt) + _mac(aead, bytes(key), bytes(ad), bytes(pt)) + bytes([pad_len - 1]) * pad_len


def cbc_encrypt(aes_key, iv, plain):
    out, c = b"", iv
    for i in range(0, len(plain), 16):
        c = o.aes_block(aes_key, bytes(a ^ b for a, b in zip(plain[i:i + 16], c)))
        out += c
    return out


def cbc_decrypt(aes_key, iv, wire):
    out, c = b"", iv
    for i in range(0, len(wire), 16):
        d = aes_decrypt_block(aes_key, wire[i:i + 16])
        out += bytes(a ^ b for a, b in zip(d, c))
        c = wire[i:i + 16]
    return out


def open_(aead, key, nonce, wire, ad):
    """(the whole decryption, data_len), or None if the reference call returns 0
    (a length that is no multiple of 16 or below mac_len + 1, wrong padding, a
    wrong MAC, a wrong nonce or AD length)."""
    _, m, _ = AEADS[aead]
    key, nonce, wire, ad = bytes(key), bytes(nonce), bytes(wire), bytes(ad)
    assert len(key) == key_len(aead)
    if len(wire) < m or len(nonce) != NONCE_LEN or len(ad) != AD_LEN:
        return None
    if len(wire) % 16 or len(wire) < m + 1:
        return None
    plain = cbc_decrypt(key[m:], nonce, wire)
    p = plain[-1]
    good = len(plain) >= m + 1 + p and all(b == p for b in plain[len(plain) - 1 - p:])
    # tls_cbc.cc:73-77: a wrong padding counts as none; the MAC then fails too
    # (or not: the record is rejected either way).
    data_len = len(plain) - m - (p + 1 if good else 0)
    mac = _mac(aead, key, ad, plain[:data_len])
    if not good or mac != plain[data_len:data_len + m]:
        return None
    return plain, data_len


@functools.lru_cache(maxsize=None)
def _kat():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_tls_cbc.json.xz")
    with lzma.open(path, "rt") as f:
        return [json.loads(line) for line in f]


def load_kat(aead):
    """The cases of the reference's vector file for `aead`
    (tests/golden/kat_tls_cbc.json.xz: one JSON record per line)."""
    return [c for c in _kat() if c["aead"] == aead]


def fixture_inputs(rec):
    """(key, nonce, pt, ad) of a ref_tls_cbc.json record (the rule of
    tests/golden/ref_tls_cbc_gen.cc: every input is derive(label + "/what"))."""
    label = rec["label"]
    return (derive(label + "/key", key_len(rec["aead"])), derive(label + "/nonce", NONCE_LEN),
            derive(label + "/pt", rec["pt_len"]), derive(label + "/ad", AD_LEN))
