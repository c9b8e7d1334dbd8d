"""The TLS 1.1 / 1.2 AES-CBC-HMAC record layer restated in plain Python, over
tests/tls_cbc_ref.py (the AEADs) -- what SSLAEADContext::Create / SealScatter /
Open (ssl/ssl_aead_ctx.cc:95-114, 226-381) and do_seal_record / tls_open_record
(ssl/tls_record.cc:117-133, 204-209, 288-299) of the reference do for a CBC
suite with an explicit IV -- and the ChaCha20 block (RFC 8439 2.3) of the
record layer's IV generator.

TEST INFRASTRUCTURE ONLY.  Pinned to the reference by
tests/golden/ref_tls_cbc_records.json (tests/test_tls_cbc_records_ref.py).
"""
import functools
import hashlib
import json
import os
import struct

import tls_cbc_ref as r
from tls_util import fill_bytes

TLS1_1_VERSION, TLS1_2_VERSION = 0x0302, 0x0303
PREFIX_LEN = 21
MAX_PLAIN = 16384
MAX_ENCRYPTED = 16384 + 320  # SSL3_RT_MAX_ENCRYPTED_LENGTH
# The lengths of the fixture: the padding edges of both MAC sizes, the
# hash-block edges (13 + len = 55, 56, 63, 64 mod 64) and the limit.
EDGE_LENGTHS = [0, 1, 11, 12, 15, 16, 17, 27, 28, 42, 43, 50, 51, 64, 255, 1350, 16383, 16384]


def ad_of(seq, typ, version):
    """GetAdditionalData with omit_length_in_ad_: 11 bytes."""
    return seq.to_bytes(8, "big") + bytes([typ]) + version.to_bytes(2, "big")


def seal_record(aead, version, enc_key, mac_key, seq, typ, pt, iv):
    """(prefix, body, suffix) -- suffix of the AEAD's tag length, without the
    zeros that fill the slot -- or None for a plaintext over 2^14 bytes."""
    if len(pt) > MAX_PLAIN:
        return None
    wire = r.seal(aead, bytes(mac_key) + bytes(enc_key), iv, pt, ad_of(seq, typ, version))
    assert wire is not None and len(wire) == len(pt) + r.tag_len(aead, len(pt))
    hdr = bytes([typ]) + version.to_bytes(2, "big") + (16 + len(wire)).to_bytes(2, "big")
    return hdr + bytes(iv), wire[:len(pt)], wire[len(pt):]


def open_record(aead, version, enc_key, mac_key, seq, prefix, fragment):
    """(type, the whole decryption, plaintext length), or None where the
    record fails.  `fragment` is what follows the IV."""
    typ, ver, hlen = prefix[0], int.from_bytes(prefix[1:3], "big"), int.from_bytes(prefix[3:5], "big")
    if ver != version or hlen != 16 + len(fragment) or 16 + len(fragment) > MAX_ENCRYPTED:
        return None
    got = r.open_(aead, bytes(mac_key) + bytes(enc_key), prefix[5:21], fragment,
                  ad_of(seq, typ, version))
    if got is None or got[1] > MAX_PLAIN:
        return None
    return typ, got[0], got[1]


def chacha20_block(key, counter, nonce_words):
    """RFC 8439 2.3: the 64-byte block of a 32-byte key, a 32-bit block counter
    and three 32-bit nonce words."""
    st = list(struct.unpack("<4I", b"expand 32-byte k")) + list(struct.unpack("<8I", bytes(key))) + \
        [counter & 0xffffffff] + [w & 0xffffffff for w in nonce_words]
    x = list(st)

    def rotl(v, c):
        return ((v << c) | (v >> (32 - c))) & 0xffffffff

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xffffffff; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xffffffff; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return struct.pack("<16I", *((a + b) & 0xffffffff for a, b in zip(x, st)))


def generated_iv(iv_key, seq):
    """The record layer's IV of sequence number seq (include/bssl_amd/tls.h)."""
    return chacha20_block(iv_key, seq & 0xffffffff, [seq >> 32, 0, 0])[:16]


@functools.lru_cache(maxsize=None)
def load_cases():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "ref_tls_cbc_records.json")
    with open(path) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def record_plaintext(length, pt_seed):
    return fill_bytes(length, pt_seed)


def body_matches(rec, body):
    """Whether `body` is the fixture record's (hex, or its SHA-256)."""
    want = rec["body"]
    if want.startswith("sha256:"):
        return hashlib.sha256(bytes(body)).hexdigest() == want[7:]
    return bytes(body).hex() == want


@functools.lru_cache(maxsize=None)
def restated_case(idx):
    """Every record of fixture case idx sealed by the restatement with the
    fixture's IVs: [(prefix, body, suffix)] -- computed once, shared."""
    c = load_cases()[idx]
    enc_key, mac_key = bytes.fromhex(c["enc_key"]), bytes.fromhex(c["mac_key"])
    out = []
    for rec in c["records"]:
        pt = record_plaintext(rec["len"], rec["pt_seed"])
        out.append(seal_record(c["aead"], c["version"], enc_key, mac_key, rec["seq"], rec["type"],
                               pt, bytes.fromhex(rec["prefix"])[5:]))
    return tuple(out)
