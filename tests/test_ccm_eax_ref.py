"""The checker of the AES-CCM / AES-EAX feature is itself checked (CPU only):
the plain Python restatement (tests/ccm_eax_ref.py) reproduces

* every known answer of the reference carried in tests/golden/kat_ccm_eax.json
  (its own vector files and the applicable Wycheproof groups), and
* every record the reference library sealed for tests/golden/ref_ccm_eax.json
  (lengths up to CCM's limit and past it, both sides of CCM's AD-length
  encoding switch, an EAX counter that carries out of its low word).

The counts are asserted, so a filter that drops cases cannot pass silently."""
import hashlib
from collections import Counter

import pytest

import ccm_eax_ref as ref
from golden_util import load

# Cases per vector file of the reference, and per Wycheproof file (valid, invalid).
FILE_CASES = {
    "crypto/cipher/test/aes_128_ccm_bluetooth_tests.txt": 25,
    "crypto/cipher/test/aes_128_ccm_bluetooth_8_tests.txt": 11,
    "crypto/cipher/test/aes_128_ccm_matter_tests.txt": 11,
    "crypto/cipher/test/aes_128_eax_test.txt": 33,
    "crypto/cipher/test/aes_256_eax_test.txt": 15,
}
WYCHEPROOF_CASES = {
    "third_party/wycheproof_testvectors/aes_ccm_test.json": (6, 0),
    "third_party/wycheproof_testvectors/aes_eax_test.json": (94, 54),
}
MSG_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1350, 4097, 65535]
AD_LENS = [0, 1, 13, 14, 15, 16, 30, 65279, 65280]


@pytest.fixture(scope="module")
def kat():
    return load("kat_ccm_eax.json")


@pytest.fixture(scope="module")
def recs():
    return load("ref_ccm_eax.json")


def test_kat_counts(kat):
    files = Counter(c["source"].split("#")[0] for c in kat)
    for f, n in FILE_CASES.items():
        assert files[f] == n, f
    for f, (valid, invalid) in WYCHEPROOF_CASES.items():
        got = Counter(c["valid"] for c in kat if c["source"].startswith(f))
        assert (got[True], got[False]) == (valid, invalid), f
    assert len(kat) == sum(FILE_CASES.values()) + sum(a + b for a, b in WYCHEPROOF_CASES.values())
    assert set(c["aead"] for c in kat) == set(ref.AEADS)


def test_restatement_matches_every_known_answer(kat):
    for c in kat:
        key, nonce, ad, pt, ct, tag = (bytes.fromhex(c[k])
                                       for k in ("key", "nonce", "ad", "pt", "ct", "tag"))
        opened = ref.open_(c["aead"], key, nonce, ct, ad, tag)
        if c["valid"]:
            assert ref.seal(c["aead"], key, nonce, pt, ad) == (ct, tag), c["source"]
            assert opened == pt, c["source"]
        else:
            assert opened is None, c["source"]


def test_reference_fixture_contents(recs):
    by = Counter(r["aead"] for r in recs)
    for aead, (mode, _, _) in ref.AEADS.items():
        nonce_lens = [13] if mode == "ccm" else [16, 12]
        for nl in nonce_lens:
            mine = [r for r in recs if r["aead"] == aead and len(r["nonce"]) == 2 * nl]
            what = lambda r: r["label"].rsplit("/", 1)[1]  # noqa: E731
            msgs = sorted(r["pt_len"] for r in mine if what(r).startswith("msg"))
            assert msgs == MSG_LENS + [65536] + ([70001] if mode == "eax" else []), (aead, nl)
            ads = [r for r in mine if what(r).startswith("ad")]
            assert sorted(r["ad_len"] for r in ads) == AD_LENS and all(r["pt_len"] == 33 for r in ads)
        over = [r for r in recs if r["aead"] == aead and r["pt_len"] > ref.CCM_MAX_INPUT]
        # CCM over its limit: the reference returned 0; EAX has no limit.
        assert all(r["ok"] == (mode == "eax") for r in over) and over
        assert all(r["ok"] for r in recs if r["aead"] == aead and r["pt_len"] <= ref.CCM_MAX_INPUT)
    assert by == {"aes-128-ccm-bluetooth": 24, "aes-128-ccm-bluetooth-8": 24,
                  "aes-128-ccm-matter": 24, "aes-128-eax": 51, "aes-256-eax": 51}
    carry = [r for r in recs if r["label"].endswith("/carry")]
    assert sorted(r["aead"] for r in carry) == ["aes-128-eax", "aes-256-eax"]
    for r in carry:
        key, nonce, _, _ = ref.fixture_inputs(r)
        # 512 bytes = 32 blocks: the counter carries out of its low 32 bits
        assert int.from_bytes(ref.eax_n(key, nonce)[12:], "big") >= 0xfffffff0 and r["pt_len"] == 512


def test_restatement_matches_every_reference_record(recs):
    for r in recs:
        key, nonce, pt, ad = ref.fixture_inputs(r)
        got = ref.seal(r["aead"], key, nonce, pt, ad)
        if not r["ok"]:
            assert got is None, r["label"]
            continue
        ct, tag = got
        if "ct" in r:
            assert (ct.hex(), tag.hex()) == (r["ct"], r["tag"]), r["label"]
        else:
            assert hashlib.sha256(ct + tag).hexdigest() == r["sha256"], r["label"]
        assert ("ct" in r) == (r["pt_len"] <= 64)
