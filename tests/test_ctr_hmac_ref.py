"""The checker of the AES-CTR-HMAC-SHA256 feature is itself checked (CPU only):
the plain Python restatement (tests/ctr_hmac_ref.py) reproduces

* every known answer of the reference carried in tests/golden/kat_ctr_hmac.json
  (its two vector files, 48 cases each), and
* every record the reference library sealed for tests/golden/ref_ctr_hmac.json
  (both sides of every 16- and 64-byte edge of the message, SHA-256's padding
  edge, the header-block edge of the AD, truncated tags).

The counts are asserted, so a filter that drops cases cannot pass silently."""
import hashlib
from collections import Counter

import pytest

import ctr_hmac_ref as ref
from golden_util import load

FILE_CASES = {
    "crypto/cipher/test/aes_128_ctr_hmac_sha256.txt": 48,
    "crypto/cipher/test/aes_256_ctr_hmac_sha256.txt": 48,
}
MSG_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 55, 56, 57, 63, 64, 65, 111, 119, 120, 121,
            127, 128, 129, 255, 256, 257, 1350, 4095, 4096, 4097]
AD_LENS = [0, 1, 35, 36, 37, 63, 64, 65, 99, 100, 101, 4097]
TAG_LENS = [1, 16, 31]
# ref_ctr_hmac_gen.cc: per AEAD, MSG_LENS x AD {0, 13}, AD_LENS x message
# {0, 57}, TAG_LENS x message {57, 1350}.
PER_AEAD = 2 * len(MSG_LENS) + 2 * len(AD_LENS) + 2 * len(TAG_LENS)


@pytest.fixture(scope="module")
def kat():
    return load("kat_ctr_hmac.json")


@pytest.fixture(scope="module")
def recs():
    return load("ref_ctr_hmac.json")


def test_kat_counts(kat):
    files = Counter(c["source"].split("#")[0] for c in kat)
    assert files == FILE_CASES
    assert len(kat) == 96
    assert set(c["aead"] for c in kat) == set(ref.AEADS)
    # what the known answers cover (and so what ref_ctr_hmac.json adds to)
    assert set(len(c["pt"]) // 2 for c in kat) == {0, 1, 15, 16, 17, 63, 64, 128}
    assert set(len(c["ad"]) // 2 for c in kat) == {0, 1, 43, 44, 45, 128}
    assert all(len(c["tag"]) == 64 and c["valid"] for c in kat)


def test_restatement_matches_every_known_answer(kat):
    for c in kat:
        key, nonce, ad, pt, ct, tag = (bytes.fromhex(c[k])
                                       for k in ("key", "nonce", "ad", "pt", "ct", "tag"))
        assert ref.seal(c["aead"], key, nonce, pt, ad) == (ct, tag), c["source"]
        assert ref.open_(c["aead"], key, nonce, ct, ad, tag) == pt, c["source"]
        bad = bytes([tag[0] ^ 1]) + tag[1:]
        assert ref.open_(c["aead"], key, nonce, ct, ad, bad) is None


def test_reference_fixture_contents(recs):
    assert len(recs) == 2 * PER_AEAD == 184
    assert Counter(r["aead"] for r in recs) == {a: PER_AEAD for a in ref.AEADS}
    assert len(set(r["label"] for r in recs)) == len(recs)
    for aead in ref.AEADS:
        mine = [r for r in recs if r["aead"] == aead]
        kind = lambda r: r["label"].split("/")[1]  # noqa: E731
        msgs = [r for r in mine if kind(r).startswith("msg")]
        for ad_len in (0, 13):
            assert sorted(r["pt_len"] for r in msgs if r["ad_len"] == ad_len) == MSG_LENS
        ads = [r for r in mine if kind(r).startswith("ad")]
        for pt_len in (0, 57):
            assert sorted(r["ad_len"] for r in ads if r["pt_len"] == pt_len) == AD_LENS
        assert all(r["tag_len"] == 32 for r in msgs + ads)
        tags = [r for r in mine if kind(r).startswith("tag")]
        assert sorted((r["tag_len"], r["pt_len"]) for r in tags) == \
            [(t, m) for t in TAG_LENS for m in (57, 1350)]
    # the edges by name: SHA-256's padding needs a block more from len % 64 = 56
    # on, and 28 + 36 = 64 header bytes fill the first hash block exactly
    assert {55, 56, 119, 120} <= set(MSG_LENS) and {35, 36, 37, 99, 100, 101} <= set(AD_LENS)


def test_restatement_matches_every_reference_record(recs):
    for r in recs:
        key, nonce, pt, ad = ref.fixture_inputs(r)
        ct, tag = ref.seal(r["aead"], key, nonce, pt, ad, r["tag_len"])
        assert len(tag) == r["tag_len"]
        if "ct" in r:
            assert (ct.hex(), tag.hex()) == (r["ct"], r["tag"]), r["label"]
        else:
            assert hashlib.sha256(ct + tag).hexdigest() == r["sha256"], r["label"]
        assert ("ct" in r) == (r["pt_len"] <= 64)
        # a truncated tag is a prefix of the full one
        assert ref.seal(r["aead"], key, nonce, pt, ad)[1][:r["tag_len"]] == tag
