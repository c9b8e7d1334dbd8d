"""The checker of the TLS AES-CBC-HMAC feature is itself checked (CPU only): the
plain Python restatement (tests/tls_cbc_ref.py)

* has a correct inverse cipher: against the reference's AES known answers
  (tests/golden/kat_aes.json) and against dec(enc(x)) == x with the oracle;
* reproduces every case of the reference's three vector files carried in
  tests/golden/kat_tls_cbc.json.xz (424 each): seal where NO_SEAL is
  absent, open everywhere, failure exactly where FAILS is set;
* reproduces every record the reference library sealed for
  tests/golden/ref_tls_cbc.json.

The counts are asserted, so a filter that drops cases cannot pass silently."""
import hashlib
from collections import Counter

import pytest

import oracle_lib as o
import tls_cbc_ref as ref
from golden_util import load

FILES = {
    "aes-128-cbc-sha1-tls": "crypto/cipher/test/aes_128_cbc_sha1_tls_tests.txt",
    "aes-256-cbc-sha1-tls": "crypto/cipher/test/aes_256_cbc_sha1_tls_tests.txt",
    "aes-128-cbc-sha256-tls": "crypto/cipher/test/aes_128_cbc_sha256_tls_tests.txt",
}
# ref_tls_cbc_gen.cc: per AEAD every length 0..130, then these.
REF_LENS = list(range(131)) + [1350, 16384, 65535, 65536, 65541]


@pytest.fixture(scope="module")
def recs():
    return load("ref_tls_cbc.json")


def test_inverse_cipher_known_answers():
    raw = [c for c in load("kat_aes.json") if c["mode"] == "Raw"]
    assert len(raw) >= 3 and {len(c["key"]) // 2 for c in raw} == {16, 24, 32}
    for c in raw:
        key, pt, ct = (bytes.fromhex(c[k]) for k in ("key", "pt", "ct"))
        assert o.aes_block(key, pt) == ct
        assert ref.aes_decrypt_block(key, ct) == pt, c["source"]


def test_inverse_cipher_inverts_the_oracle():
    for key_len in (16, 32):
        for i in range(64):
            key = ref.derive(f"inv/{key_len}/{i}/key", key_len)
            x = ref.derive(f"inv/{key_len}/{i}/block", 16)
            assert ref.aes_decrypt_block(key, o.aes_block(key, x)) == x
            assert o.aes_block(key, ref.aes_decrypt_block(key, x)) == x
    iv, key = ref.derive("inv/iv", 16), ref.derive("inv/cbc", 32)
    msg = ref.derive("inv/msg", 160)
    assert ref.cbc_decrypt(key, iv, ref.cbc_encrypt(key, iv, msg)) == msg


@pytest.mark.parametrize("aead", list(FILES))
def test_restatement_matches_every_vector_case(aead):
    kat = ref.load_kat(aead)
    assert len(kat) == 424
    assert sum(c["no_seal"] for c in kat) == 324 and sum(c["fails"] for c in kat) == 259
    assert {c["source"].split("#")[0] for c in kat} == {FILES[aead]}
    assert all(c["aead"] == aead and c["tag_len"] == ref.mac_len(aead) for c in kat)
    sealed = opened = failed = 0
    for c in kat:
        key, nonce, ad, pt, ct, tag = (bytes.fromhex(c[k])
                                       for k in ("key", "nonce", "ad", "pt", "ct", "tag"))
        if not c["no_seal"]:
            assert ref.seal(aead, key, nonce, pt, ad) == ct + tag, c["source"]
            assert len(tag) == ref.tag_len(aead, len(pt))
            sealed += 1
        got = ref.open_(aead, key, nonce, ct + tag, ad)
        if c["fails"]:
            assert got is None, c["source"]
            failed += 1
        else:
            plain, data_len = got
            assert plain[:data_len] == pt and len(plain) == len(ct + tag), c["source"]
            opened += 1
    assert (sealed, opened, failed) == (100, 165, 259)


def test_reference_fixture_contents(recs):
    assert len(recs) == 3 * len(REF_LENS) == 408
    assert Counter(r["aead"] for r in recs) == {a: len(REF_LENS) for a in ref.AEADS}
    assert len(set(r["label"] for r in recs)) == len(recs)
    for aead in ref.AEADS:
        mine = [r for r in recs if r["aead"] == aead]
        assert sorted(r["pt_len"] for r in mine) == REF_LENS
        # every residue of (len + mac_len) mod 16, so every padding length 1..16
        assert {r["tag_len"] - ref.mac_len(aead) for r in mine} == set(range(1, 17))
        assert all(("wire" in r) == (r["pt_len"] <= 64) for r in mine)
    # the edges by name: 13 + 43 = 56 (SHA's padding needs a second block), 13 +
    # 51 = 64 (the first hash block full), and the 16-bit length wrap
    assert {42, 43, 50, 51, 52, 65535, 65536, 65541} <= set(REF_LENS)


def test_restatement_matches_every_reference_record(recs):
    for r in recs:
        aead = r["aead"]
        key, nonce, pt, ad = ref.fixture_inputs(r)
        wire = ref.seal(aead, key, nonce, pt, ad)
        assert len(wire) == r["pt_len"] + r["tag_len"]
        assert r["tag_len"] == ref.tag_len(aead, r["pt_len"])
        if "wire" in r:
            assert wire.hex() == r["wire"], r["label"]
        else:
            assert hashlib.sha256(wire).hexdigest() == r["sha256"], r["label"]
        if r["pt_len"] <= 1350:  # (the inverse cipher in Python is slow)
            plain, data_len = ref.open_(aead, key, nonce, wire, ad)
            assert data_len == len(pt) and plain == ref.plain_of(aead, key, pt, ad)


def test_open_accepts_any_padding_length_and_rejects_the_rest():
    aead = "aes-128-cbc-sha256-tls"
    key, nonce, ad = ref.derive("pad/key", 48), ref.derive("pad/nonce", 16), ref.derive("pad/ad", 11)
    pt = ref.derive("pad/pt", 37)
    for pad_len in (11, 27, 251):  # 37 + 32 + 11 = 80
        wire = ref.seal(aead, key, nonce, pt, ad, pad_len=pad_len)
        plain, data_len = ref.open_(aead, key, nonce, wire, ad)
        assert data_len == 37 and plain[:37] == pt and len(plain) == 37 + 32 + pad_len
    assert ref.open_(aead, key, nonce, wire[:-16], ad) is None
    assert ref.open_(aead, key, nonce, wire[:32], ad) is None  # below mac_len + 1
    assert ref.open_(aead, key, nonce, wire[:-1], ad) is None
    assert ref.open_(aead, key, nonce, wire, ad + b"x") is None
    assert ref.seal(aead, key, nonce[:12], pt, ad) is None
