"""CPU tests that pin the Python restatement of the TLS 1.1 / 1.2 AES-CBC-HMAC
record layer (tests/tls_cbc_records_util.py) to the reference: the records of
tests/golden/ref_tls_cbc_records.json were sealed and opened by the reference's
own SSLAEADContext (tests/golden/ref_tls_cbc_records_gen.cc).  No GPU call."""
import pytest

import tls_cbc_records_util as u

CASES = u.load_cases()
IDS = [f"{c['aead']}-{c['version']:04x}-seq{c['seq0']:x}" for c in CASES]


def test_fixture_covers_the_stated_cases():
    assert len(CASES) == 12
    assert {(c["aead"], c["version"], c["seq0"]) for c in CASES} == {
        (a, v, s) for a in ("aes-128-cbc-sha1-tls", "aes-256-cbc-sha1-tls", "aes-128-cbc-sha256-tls")
        for v in (0x0302, 0x0303) for s in (0, 0x1234567890)}
    for c in CASES:
        assert [r["len"] for r in c["records"]] == u.EDGE_LENGTHS
        assert [r["seq"] for r in c["records"]] == list(range(c["seq0"], c["seq0"] + 18))
        assert [r["type"] for r in c["records"]] == [(23, 22, 21)[i % 3] for i in range(18)]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_restatement_seals_the_reference_records(idx):
    c = CASES[idx]
    for rec, got in zip(c["records"], u.restated_case(idx)):
        prefix, body, suffix = got
        assert prefix.hex() == rec["prefix"], rec["len"]
        assert u.body_matches(rec, body), rec["len"]
        assert suffix.hex() == rec["suffix"], rec["len"]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_restatement_opens_the_reference_records(idx):
    c = CASES[idx]
    enc_key, mac_key = bytes.fromhex(c["enc_key"]), bytes.fromhex(c["mac_key"])
    for rec, (prefix, body, suffix) in zip(c["records"], u.restated_case(idx)):
        # (the body is the restatement's where the fixture stores a digest:
        # the test above showed them equal)
        got = u.open_record(c["aead"], c["version"], enc_key, mac_key, rec["seq"],
                            bytes.fromhex(rec["prefix"]), body + bytes.fromhex(rec["suffix"]))
        assert got is not None, rec["len"]
        typ, plain, n = got
        assert typ == rec["type"] and n == rec["len"]
        assert plain[:n] == u.record_plaintext(rec["len"], rec["pt_seed"])


def test_open_record_rejects_what_the_record_layer_rejects():
    c = CASES[0]
    enc_key, mac_key = bytes.fromhex(c["enc_key"]), bytes.fromhex(c["mac_key"])
    rec = c["records"][5]
    prefix, body, suffix = u.restated_case(0)[5]
    args = (c["aead"], c["version"], enc_key, mac_key)
    assert u.open_record(*args, rec["seq"], prefix, body + suffix) is not None
    assert u.open_record(*args, rec["seq"] + 1, prefix, body + suffix) is None
    wrong_version = prefix[:1] + b"\x03\x03" + prefix[3:]
    assert u.open_record(*args, rec["seq"], wrong_version, body + suffix) is None
    wrong_length = prefix[:3] + b"\x00\x10" + prefix[5:]
    assert u.open_record(*args, rec["seq"], wrong_length, body + suffix) is None
    wrong_type = bytes([prefix[0] ^ 1]) + prefix[1:]
    assert u.open_record(*args, rec["seq"], wrong_type, body + suffix) is None


def test_chacha20_block_is_rfc_8439():
    # RFC 8439 2.3.2: key 00..1f, block counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00.
    block = u.chacha20_block(bytes(range(32)), 1, [0x09000000, 0x4a000000, 0])
    assert block.hex() == (
        "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
        "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    # The record layer's IV: counter (uint32)seq, first nonce word seq >> 32.
    assert u.generated_iv(bytes(range(32)), (0x09000000 << 32) | 1) == \
        u.chacha20_block(bytes(range(32)), 1, [0x09000000, 0, 0])[:16]
    assert u.generated_iv(bytes(32), 0xffffffff) != u.generated_iv(bytes(32), 0x100000000)
