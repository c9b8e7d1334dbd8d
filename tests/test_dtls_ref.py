"""CPU tests of the DTLS model (tests/dtls_util.py) that the GPU tests compare
BSSL_AMD_DTLS_AEAD against: sequence reconstruction at its edges, the DTLS 1.2
records against the TLS restatement that is pinned to the reference's golden
records, the model's own round trip, and where reconstruction against the
batch's start differs from the reference's record-by-record one."""
import random

import pytest

import dtls_util as d
import oracle_lib as o
import tls_util

AEADS = (("aes-128-gcm", 16), ("aes-256-gcm", 32), ("chacha20-poly1305", 32))


def _params(version, aead, key_len, epoch=1, seed=0):
    rnd = random.Random(1000 * seed + key_len + version)
    key = bytes(rnd.randrange(256) for _ in range(key_len))
    iv = bytes(rnd.randrange(256) for _ in range(d.iv_len(version, aead)))
    sn = bytes(rnd.randrange(256) for _ in range(key_len)) if version == d.DTLS1_3 else None
    return d.Params(version, aead, key, iv, sn, epoch)


# (wire, mask, max) -> sequence: the points the reference's own unit test
# exercises, for both masks.
EDGES = [
    # start of the epoch
    (0, 0xff, 0, 0), (1, 0xff, 0, 1), (0xff, 0xff, 0, 0xff),
    (0, 0xffff, 0, 0), (1, 0xffff, 0, 1), (0xff, 0xffff, 0, 0xff),
    # carry
    (0, 0xff, 0xff, 0x100), (0, 0xffff, 0xffff, 0x10000),
    # decrement
    (0, 0xff, 0x210, 0x200), (0xff, 0xff, 0x200, 0x1ff),
    (0, 0xffff, 0x21000, 0x20000), (0xffff, 0xffff, 0x20000, 0x1ffff),
    # the tie goes to the larger value
    (0x80, 0xff, 0x100, 0x180), (0x81, 0xff, 0x100, 0x181), (0x82, 0xff, 0x100, 0x82),
    (0x8000, 0xffff, 0x10000, 0x18000), (0x8001, 0xffff, 0x10000, 0x18001),
    (0x8002, 0xffff, 0x10000, 0x8002),
    # the clamp at 2^48 - 1
    (0, 0xff, d.MAX_SEQ, d.MAX_SEQ - 255), (0, 0xffff, d.MAX_SEQ, d.MAX_SEQ - 65535),
    (0xff, 0xff, d.MAX_SEQ, d.MAX_SEQ), (0xffff, 0xffff, d.MAX_SEQ - 5, d.MAX_SEQ),
]


@pytest.mark.parametrize("wire,mask,max_seq,want", EDGES)
def test_reconstruction_edges(wire, mask, max_seq, want):
    got = d.reconstruct_seqnum(wire, mask, max_seq)
    assert got == want
    assert got & mask == wire and 0 <= got <= d.MAX_SEQ


def test_reconstruction_is_the_closest_congruent_value():
    rnd = random.Random(7)
    for _ in range(2000):
        mask = rnd.choice((0xff, 0xffff))
        max_seq = rnd.choice((rnd.randrange(0, 70000), rnd.randrange(0, d.MAX_SEQ + 1),
                              d.MAX_SEQ - rnd.randrange(0, 70000)))
        wire = rnd.randrange(mask + 1)
        got = d.reconstruct_seqnum(wire, mask, max_seq)
        cands = [c for c in range(got - 2 * (mask + 1), got + 3 * (mask + 1), mask + 1)
                 if 0 <= c <= d.MAX_SEQ]
        best = min(cands, key=lambda c: (abs(c - (max_seq + 1)), -c))
        assert got == best, (wire, mask, max_seq)


def test_window_is_the_reference_bitmap():
    w = d.Window()
    assert w.bitmap() == bytes(32) and not w.should_discard(0)
    w.record(0)
    assert w.should_discard(0) and w.bitmap()[0] == 1
    w.record(5)
    assert w.max_seq == 5 and w.bits == 0b100001
    assert w.should_discard(5) and w.should_discard(0) and not w.should_discard(3)
    w.record(5 + 255)
    assert not w.should_discard(5 + 255 - 255 + 1) and w.should_discard(5)  # 5: still marked
    assert w.should_discard(4) is True                                       # older than max - 255
    w.record(5 + 255 + 256)                                                  # a jump of 256 clears
    assert w.bits == 1
    assert d.Window.from_bitmap(w.max_seq, w.bitmap()).bits == w.bits


@pytest.mark.parametrize("aead,key_len", AEADS)
def test_dtls12_records_are_the_tls_restatement_with_the_combined_number(aead, key_len):
    """Body and explicit nonce equal tls_util.tls_seal_restated run with seq =
    epoch << 48 | sequence: the nonce is formed alike.  That restatement writes
    03 03 into its additional data whatever version it is given, so its tag
    is not DTLS's; the tag is checked against the oracle under the
    restatement's AD with the version bytes replaced by fe fd."""
    p = _params(d.DTLS1_2, aead, key_len, epoch=3)
    seq0 = 0xfffe
    contents = [tls_util.fill_bytes(n, 40 + n) for n in (0, 1, 16, 63, 1350)]
    types = [23, 22, 21, 23, 23]
    got = d.seal(p, seq0, contents, types)
    ref = tls_util.tls_seal_restated(tls_util.TLS1_2_VERSION, aead, p.key, p.iv,
                                     p.combined(seq0), contents, types)
    for i, (g, r, pt, typ) in enumerate(zip(got, ref, contents, types)):
        assert g["body"] == r[1]
        assert g["prefix"][13:] == r[0][5:]                  # the explicit nonce
        assert g["prefix"][3:11] == p.combined(seq0 + i).to_bytes(8, "big")
        ad = p.combined(seq0 + i).to_bytes(8, "big") + bytes([typ, 0xfe, 0xfd]) + \
            len(pt).to_bytes(2, "big")
        aid = o.CHACHA20_POLY1305 if aead == "chacha20-poly1305" else o.AES_GCM
        ok, ct, tag = o.seal(aid, p.key, p.nonce(seq0 + i), pt, ad)
        assert ok and ct == g["body"] and tag == g["tag"]
        assert len(g["prefix"]) == p.prefix_len
        assert int.from_bytes(g["prefix"][11:13], "big") == p.explicit + len(pt) + 16


@pytest.mark.parametrize("version", (d.DTLS1_2, d.DTLS1_3))
@pytest.mark.parametrize("aead,key_len", AEADS)
def test_model_round_trip(version, aead, key_len):
    p = _params(version, aead, key_len, epoch=2)
    contents = [tls_util.fill_bytes(n, n) for n in (0, 1, 14, 15, 16, 17, 200)]
    types = [23, 22, 21, 23, 23, 20, 23]
    seq0 = 0xfffd  # crosses 0xffff -> 0x10000
    sealed = d.seal(p, seq0, contents, types)
    w = d.Window(seq0 - 1)
    res = d.open_batch(p, w, [(r["prefix"], r["body"], r["tag"]) for r in sealed])
    for i, (r, pt, typ) in enumerate(zip(res, contents, types)):
        assert r["status"] == 1 and r["type"] == typ and r["number"] == p.combined(seq0 + i)
        assert r["out"][:len(pt)] == pt
        assert r["out_len"] == len(pt)
    assert w.max_seq == seq0 + 6 and w.bits & 0x7f == 0x7f
    # Replayed: every one is refused, the window is unchanged.
    before = (w.max_seq, w.bits)
    res = d.open_batch(p, w, [(r["prefix"], r["body"], r["tag"]) for r in sealed])
    assert all(r["status"] == 0 and r["out"] == bytes(len(r["out"])) for r in res)
    assert (w.max_seq, w.bits) == before


def test_dtls13_header_forms_and_padding_round_trip():
    p = _params(d.DTLS1_3, "aes-128-gcm", 16, epoch=5)
    recs, want = [], []
    s = 300
    for seq16 in (True, False):
        for with_len in (True, False):
            for pad in (0, 1, 15):
                content = tls_util.fill_bytes(20 + pad, s)
                recs.append(d.build_record13(p, s, content, 23, pad, seq16, with_len))
                want.append((s, content))
                s += 1
    w = d.Window(299)
    res = d.open_batch(p, w, recs)
    for r, (s, content) in zip(res, want):
        assert r["status"] == 1 and r["number"] == p.combined(s) and r["type"] == 23
        assert r["out_len"] == len(content) and r["out"][:len(content)] == content
    # The reject paths fail alone.
    bad = [d.build_record13(p, 400, b"x", 23, cbit=True),
           d.build_record13(p, 401, b"x", 23, epoch_bits=(p.epoch + 1) & 3),
           d.build_record13(p, 402, b"", 0),
           d.build_record13(p, 403, b"x", 23, stated_delta=1)]
    good = d.build_record13(p, 404, b"y", 22)
    res = d.open_batch(p, w, bad + [good])
    assert [r["status"] for r in res] == [0, 0, 0, 0, 1]
    assert [r["number"] for r in res[:2]] == [0, 0] and res[2]["number"] == p.combined(402)
    assert w.max_seq == 404


def test_batch_start_reconstruction_against_the_record_by_record_model():
    """Inside -step/2 < s - (M0 + 1) <= step/2 the two agree; an 8-bit batch
    that runs past it does not: the reference follows the records, the batch
    form reconstructs the late ones a step too low."""
    p = _params(d.DTLS1_3, "chacha20-poly1305", 32, epoch=1)
    m0 = 1000

    def run(seqs, per_record):
        recs = [d.build_record13(p, s, b"data", 23, seq16=False) for s in seqs]
        w = d.Window(m0)
        return d.open_batch(p, w, recs, per_record=per_record), w

    # In range for both: 120 records reordered within groups of 16, so that
    # the record-by-record maximum is never far from the record at hand either.
    rnd = random.Random(3)
    inside = []
    for g in range(m0 + 1 - 8, m0 + 1 + 112, 16):
        group = list(range(g, g + 16))
        rnd.shuffle(group)
        inside += group
    a, wa = run(inside, False)
    b, wb = run(inside, True)
    assert a == b and (wa.max_seq, wa.bits) == (wb.max_seq, wb.bits)
    assert all(r["status"] == 1 for r in a)
    outside = list(range(m0 + 1, m0 + 1 + 300))
    a, wa = run(outside, False)
    b, wb = run(outside, True)
    assert all(r["status"] == 1 for r in b) and wb.max_seq == m0 + 300
    assert [r["status"] for r in a] == [1] * 129 + [0] * 171
    assert wa.max_seq == m0 + 129
