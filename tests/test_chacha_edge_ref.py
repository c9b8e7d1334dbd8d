"""chacha_edge_util.py against the CPU oracle: the Python Poly1305, and every
solved record that test_chacha_edge_gpu.py runs -- each target class at each
length, for the committed seeds, none left out -- sealed again by the oracle."""
import numpy as np
import pytest

import chacha_edge_util as u
import oracle_lib as o
import tls_util
from golden_util import load


def test_poly_acc_is_the_oracles_poly1305():
    rng = np.random.default_rng(1)
    for n_ad, n_ct in [(0, 0), (0, 1), (1, 0), (13, 1350), (16, 64), (17, 63), (80, 4113)]:
        otk = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        ad = rng.integers(0, 256, n_ad, dtype=np.uint8).tobytes()
        ct = rng.integers(0, 256, n_ct, dtype=np.uint8).tobytes()
        h, r, s = u.poly_acc(otk, ad, ct)
        assert 0 <= h < u.P and (r, s) == u.poly_key(otk)
        msg = u.pad16(ad) + u.pad16(ct) + len(ad).to_bytes(8, "little") + len(ct).to_bytes(8, "little")
        assert u.tag_of(h, s) == o.poly1305(otk, msg), (n_ad, n_ct)
    for c in load("kat_poly1305.json"):
        key, msg = bytes.fromhex(c["key"]), bytes.fromhex(c["input"])
        h, _, s = u.poly_acc_msg(key, msg)
        assert u.tag_of(h, s).hex() == c["mac"], c["source"]


def test_length_grid():
    assert len(u.LENS) == 96 and len(set(u.LENS)) == 96 and max(u.LENS) == 5 * 64 + 63
    assert {x % 64 for x in u.LENS} == set(u.R) and {x // 64 for x in u.LENS} == set(range(6))
    # every store-width residue of the last block, every count of tail blocks
    assert {x % 4 for x in u.R} == {0, 1, 2, 3}
    assert {(x + 15) // 16 % 4 for x in u.LENS} == {0, 1, 2, 3}
    assert {(a + 15) // 16 for a in u.AD_LENS} == set(range(6))
    assert {x // 64 for x in u.LONG} == {21, 64}


def test_target_classes():
    s = 0x123456789abcdef0fedcba9876543210
    t = u.targets(s)
    assert [name for name, _ in t] == u.TARGET_NAMES and len(t) == u.NUM_TARGETS
    assert all(0 <= v < u.P for _, v in t) and len({v for _, v in t}) == len(t)
    d = dict(t)
    for name in ("tag00", "tag00+2^128", "tag00+2^129"):
        assert u.tag_of(d[name], s) == bytes(16)
    for name in ("tagff", "tagff+2^128", "tagff+2^129"):
        assert u.tag_of(d[name], s) == b"\xff" * 16
    assert (d["carry1"] + s % (1 << 32)) == 1 << 32


def _reseal(aead, key, pts, ads, nonces, cts, tags, names):
    """The oracle seals the solved (pt, ad) to exactly the solved ct and tag."""
    for i, name in enumerate(names):
        ok, ct, tag = o.seal(u.ORACLE_ID[aead], key, nonces[i], pts[i], ads[i])
        assert ok and ct == cts[i] and tag == tags[i], (aead, i, name, len(pts[i]))
        if name.startswith("tag00"):
            assert tag == bytes(16)
        if name.startswith("tagff"):
            assert tag == b"\xff" * 16


def _every_class_at_every_length(lens, names):
    assert {(n, c) for n, c in zip(lens, names)} == {(n, c) for n in set(lens)
                                                      for c in u.TARGET_NAMES}


@pytest.mark.parametrize("aead", u.AEADS)
@pytest.mark.parametrize("batch", sorted(u.SOLVED))
def test_solved_batches(aead, batch):
    lens, ad_len, seed = u.SOLVED[batch]
    key = u.key_of()
    pts, ads, nonces, cts, tags, names = u.solved_batch(aead, key, lens, ad_len, seed)
    assert [len(p) for p in pts] == lens and len(set(nonces)) == len(lens)
    _every_class_at_every_length(lens, names)
    for n in set(lens):
        assert 16 * u.free_block_of(n) + 64 <= n  # a whole unit, not the tail
    _reseal(aead, key, pts, ads, nonces, cts, tags, names)


def test_solved_tls_records():
    key, iv = u.key_of(), bytes(range(1, 13))
    recs, types, cts, tags, names = u.tls_solved_batch(key, iv)
    _every_class_at_every_length(u.TLS_SOLVED_LENS, names)
    expect = tls_util.tls_seal_restated(0x0304, "chacha20-poly1305", key, iv, 0, recs, types)
    for i, (pre, body, suf) in enumerate(expect):
        assert body + suf == cts[i] + tags[i], (i, names[i])
        assert pre == u.tls13_nonce_ad(iv, i, len(recs[i]))[1]


@pytest.mark.parametrize("aead", u.AEADS)
@pytest.mark.parametrize("nblk", u.ONE_SOLVED_NBLK)
def test_solved_single_records(aead, nblk):
    key = u.key_of()
    ad_len, n = u.one_lengths(nblk, False)
    assert (ad_len + 15) // 16 + (n + 15) // 16 + 1 == nblk
    cases = u.one_solved(aead, key, nblk, nblk)
    assert [c[0] for c in cases] == u.TARGET_NAMES
    names, nonces, ads, pts, cts, tags = zip(*cases)
    _reseal(aead, key, pts, ads, nonces, cts, tags, names)


def test_single_record_lengths():
    for nblk in u.ONE_NBLK + (2049,):
        for odd in (False, True):
            ad_len, n = u.one_lengths(nblk, odd)
            assert (ad_len + 15) // 16 + (n + 15) // 16 + 1 == nblk and n <= u.ONE_MAX_LEN
            assert (ad_len % 16, n % 16) == ((1, 1) if odd else (0, 0))
    # every chunk size c = 1..8 of both chunk counts, with pad = 0 and pad = T c - 1 .. c
    shapes = set()
    for nblk in u.ONE_NBLK:
        t = 64 if nblk <= 512 else 256
        c = (nblk + t - 1) // t
        shapes.add((t, c, t * c - nblk == 0))
    assert {(t, c) for t, c, _ in shapes} == {(64, c) for c in range(1, 9)} | \
        {(256, c) for c in range(3, 9)}
    assert all((t, c, True) in shapes for t, c, _ in shapes)


@pytest.mark.parametrize("aead", u.AEADS)
def test_ones_and_zeros_contents(aead):
    key, rng = u.key_of(), np.random.default_rng(5)
    for kind, byte in (("ones", 0xff), ("zeros", 0)):
        for n, ad_len in ((4 * 64 + 49, 13), (1, 0), (0, 17), (4113, 80)):
            nonce = u.rand_nonces(aead, 1, rng)[0]
            pt, ad = u.content(kind, aead, key, nonce, n, ad_len, rng)
            ok, ct, _ = o.seal(u.ORACLE_ID[aead], key, nonce, pt, ad)
            assert ok and ct == bytes([byte]) * n and ad == bytes([byte]) * ad_len
