"""CPU tests of the TLS 1.3 padding restatement (tests/tls13_pad_util.py): with
no padding it is tls_seal_restated byte for byte, and so the reference's own
TLS 1.3 records (tests/golden/ref_tls.json); the oracle opens what it seals
and strip returns content and type; strip on a table of edge cases."""
import hashlib
import random

import pytest

import tls13_pad_util as p
import tls_util
from golden_util import load

CASES = [c for c in load("ref_tls.json") if c["version"] == 0x0304]
IDS = [f"{c['aead']}-seq{c['seq0']:x}" for c in CASES]

# (fragment, expected strip result): the cases the GPU strip is held to.
STRIP_TABLE = [
    (b"", None),
    (b"\x00", None),
    (bytes(16), None), (bytes(17), None), (bytes(1025), None), (bytes(16385), None),
    (b"\x17", (0, 23)),                          # empty content
    (b"\x17" + bytes(40), (0, 23)),              # ... and padding
    (b"abc\x16", (3, 22)),
    (b"abc\x00\x00\x15", (5, 21)),               # content ending in zeros
    (b"abc\x00\x00\x15" + bytes(2000), (5, 21)),
    (b"\x01" * 16384 + b"\x17", (16384, 23)),    # the largest fragment
    (bytes(16384) + b"\x17", (16384, 23)),
    (b"\x17" + bytes(16384), (0, 23)),
    (b"\x01" * 16385 + b"\x17", None),           # one over (tls_record.cc:204-209)
    (b"\x17" + bytes(16385), None),
    (b"\xff", (0, 255)),
]


def test_there_are_tls13_fixture_cases():
    assert len(CASES) >= 3


@pytest.mark.parametrize("frag,want", STRIP_TABLE,
                         ids=[f"{i}-len{len(f)}" for i, (f, _) in enumerate(STRIP_TABLE)])
def test_strip_table(frag, want):
    assert p.strip(frag) == want


def test_strip_finds_the_type_at_every_position():
    for f in (1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025):
        for k in range(f):
            frag = bytearray(f)
            frag[k] = 22
            assert p.strip(frag) == (k, 22)
            if k:
                frag[0] = 9  # content before it changes nothing
                assert p.strip(frag) == (k, 22)


def test_fragment_len_rules():
    assert p.fragment_len(0) == 1 and p.fragment_len(16384) == 16385
    assert p.fragment_len(16385) is None
    assert p.fragment_len(16384, 1) is None and p.fragment_len(16383, 1) == 16385
    assert p.fragment_len(10, 2 ** 32 - 1) is None
    for block in (16, 64, 512):
        for m in (1, 3):
            assert p.fragment_len(m * block - 2, block=block) == m * block      # L + 1 one below
            assert p.fragment_len(m * block - 1, block=block) == m * block      # at
            assert p.fragment_len(m * block, block=block) == (m + 1) * block    # one above
    for block in (0, 1):
        assert p.fragment_len(100, block=block) == 101
    assert p.fragment_len(16384, block=512) == 16385  # capped at the limit
    assert p.fragment_len(0, block=16385) == 16385 and p.fragment_len(0, block=2 ** 32 - 1) == 16385


def _body_matches(golden, body):
    if golden.startswith("sha256:"):
        return hashlib.sha256(body).hexdigest() == golden[7:]
    return body.hex() == golden


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_unpadded_is_the_restated_seal_and_the_fixture(case):
    key, iv = bytes.fromhex(case["key"]), bytes.fromhex(case["fixed_iv"])
    recs = [tls_util.fill_bytes(r["len"], r["pt_seed"]) for r in case["records"]]
    types = [r["type"] for r in case["records"]]
    got = p.seal_padded(case["aead"], key, iv, case["seq0"], recs, types, [0] * len(recs))
    want = tls_util.tls_seal_restated(0x0304, case["aead"], key, iv, case["seq0"], recs, types)
    for r, g, w in zip(case["records"], got, want):
        if w is None:
            assert g is None
            continue
        pre, frag, tag = g
        assert pre + frag + tag == w[0] + w[1] + w[2], r["seq"]
        assert pre.hex() == r["prefix"], r["seq"]
        assert _body_matches(r["body"], frag[:-1]), r["seq"]
        assert (frag[-1:] + tag).hex() == r["suffix"], r["seq"]


@pytest.mark.parametrize("aead", ["aes-128-gcm", "aes-256-gcm", "chacha20-poly1305"])
def test_open_of_padded_records_returns_content_and_type(aead):
    rng = random.Random(len(aead))
    key, iv = rng.randbytes(16 if "128" in aead else 32), rng.randbytes(12)
    lens = [0, 1, 15, 16, 17, 1350, 16383, 16384]
    pads = [0, 1, 14, 15, 16, 17, 1023, 1024, 1025]
    records, types, pp = [], [], []
    for L in lens:
        for pad in pads + [16384 - L]:
            if L + 1 + pad <= p.MAX_FRAGMENT:
                content = rng.randbytes(L)
                if L and rng.random() < 0.5:
                    content = content[:-1] + b"\x00"  # content may end in zeros
                records.append(content)
                types.append(rng.choice([21, 22, 23]))
                pp.append(pad)
    seq0 = (1 << 40) + 5
    sealed = p.seal_padded(aead, key, iv, seq0, records, types, pp)
    for i, (s, content, typ, pad) in enumerate(zip(sealed, records, types, pp)):
        pre, frag, tag = s
        assert len(frag) == len(content) + 1 + pad and pre == p.header(len(frag))
        pt, n, t = p.open_padded(aead, key, iv, seq0 + i, pre, frag, tag)
        assert pt == content + bytes([typ]) + bytes(pad) and (n, t) == (len(content), typ)
        # Failures: tag, header type, version, length, the wrong sequence number.
        assert p.open_padded(aead, key, iv, seq0 + i, pre, frag, bytes([tag[0] ^ 1]) + tag[1:]) is None
        assert p.open_padded(aead, key, iv, seq0 + i + 1, pre, frag, tag) is None
    pre, frag, tag = sealed[3]
    for bad in (b"\x16" + pre[1:], pre[:1] + b"\x03\x01" + pre[3:],
                pre[:4] + bytes([pre[4] ^ 1])):
        assert p.open_padded(aead, key, iv, seq0 + 3, bad, frag, tag) is None


def test_records_that_cannot_be_sealed():
    key, iv = bytes(16), bytes(12)
    got = p.seal_padded("aes-128-gcm", key, iv, 0,
                        [bytes(16385), bytes(16384), b"x", b"y", b"z"], [23, 23, 23, 0, 23],
                        [0, 1, 2 ** 32 - 1, 0, 0])
    assert got[:4] == [None] * 4 and got[4] is not None
