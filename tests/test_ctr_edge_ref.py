"""The crafted counter-edge inputs (tests/ctr_edge_util.py) on the CPU: the
constructions are pinned independently of any kernel -- the keystream block at
index i equals AES of the predicted counter block, through every wrap and
carry -- and the oracle and the Python EAX restatement are pinned at these
edges against records the reference library sealed
(tests/golden/ref_ctr_edge.json, make_golden_ctr_edge.py).

ChaCha20-Poly1305, AES-CTR-HMAC and AES-CCM have no reachable counter edge
(32-bit counters from 0 or 1 with record limits below 2^32 blocks; CCM's
L = 2 with its 65535-byte cap is tested elsewhere): nothing here for them.
"""
import collections

import pytest

import ccm_eax_ref
import ctr_edge_util as u
import oracle_lib as o
from ccm_eax_ref import derive
from golden_util import load

LANES = (2, 4, 8, 16)
NB = 260  # blocks: every fixed position (up to 257) and "last" and "mid" beyond them


def _keystream(ct, pt):
    return [u.xor(ct[i:i + 16], pt[i:i + 16]) for i in range(0, len(pt), 16)]


def test_gf_inverse_and_nonce_solver():
    key = derive("edge-ref/solver", 16)
    h = o.aes_block(key, bytes(16))
    assert u.gf_mul(u.gf_inv(h), h) == u.ONE
    assert u.gf_mul(u.ONE, h) == h
    # The solved nonces hash back to the chosen J0 (GHASH restated on gf_mul).
    j0 = derive("edge-ref/j0", 16)
    for first in (None, derive("edge-ref/first", 16)):
        nonce = u.gcm_nonce_for(key, j0, first)
        assert len(nonce) == (16 if first is None else 32)
        y = bytes(16)
        for blk in [nonce[i:i + 16] for i in range(0, len(nonce), 16)] + \
                [bytes(8) + (8 * len(nonce)).to_bytes(8, "big")]:
            y = u.gf_mul(u.xor(y, blk), h)
        assert y == j0


def test_counter_classes_hit_their_edges():
    """The counter values around block w are the ones the class names."""
    for cls, edge in u.EDGE.items():
        for w in (0, 1, 7, 256):
            j0 = bytes(12) + u.gcm_c0(cls, w, NB).to_bytes(4, "big")
            assert u.gcm_counter_block(j0, w)[12:] == (edge & u.M32).to_bytes(4, "big")
            if w:
                assert u.gcm_counter_block(j0, w - 1)[12:] == (edge - 1).to_bytes(4, "big")
                tag = u.siv_c(cls, w).to_bytes(4, "little") + bytes(12)
                assert u.siv_counter_block(tag, w)[:4] == (edge & u.M32).to_bytes(4, "little")
                assert u.siv_counter_block(tag, w - 1)[:4] == (edge - 1).to_bytes(4, "little")
    j0 = bytes(12) + u.gcm_c0("control", None, NB).to_bytes(4, "big")
    assert u.gcm_counter_block(j0, NB - 1)[12:] == b"\xff" * 4
    for cls, bits in (("ones64", 64), ("ones96", 96), ("ones128", 128)):
        n = int.from_bytes(u.eax_n_target(cls, 5, "edge-ref/n"), "big")
        assert (n + 5) % (1 << bits) == (1 << bits) - 1
        assert (n + 6) % (1 << 128) % (1 << bits) == 0
        assert (n + 6) % (1 << 128) == (0 if bits == 128 else ((n >> bits) + 1) << bits)


def test_plans_cover_every_case():
    for kind in ("gcm", "siv", "eax"):
        for lanes in ((4,), (8, 16), LANES):
            batches = u.plan_row(kind, [NB] * 20, lanes)
            seen = {c[:2] for b in batches for c in b}
            assert seen == set(u.all_cases(kind, lanes))
            assert len(batches) == -(-len(seen) // 20)
    # short records take only what fits; a case no record is long enough for is not asked for
    (b,) = u.plan_row("gcm", [1, 2, 3] * 12, (2,))
    assert all(c[2] is None or c[2] < nb for c, nb in zip(b, [1, 2, 3] * 12))
    assert {c[1] for c in b} == {0, 1, 2, "last", "mid", None}


@pytest.mark.parametrize("aead", list(u.GCM_KEYLEN))
def test_gcm_keystream_follows_inc32(aead):
    key = derive("edge-ref/" + aead, u.GCM_KEYLEN[aead])
    pt = u.data(1, 16 * NB - 5)  # (a partial last block)
    (cases,) = u.plan_row("gcm", [NB] * len(u.all_cases("gcm", LANES)), LANES, max_batches=1)
    assert {c[0] for c in cases} == set(u.GCM_CLASSES)
    for k, case in enumerate(cases):
        label = f"edge-ref/{aead}/{k}"
        first = derive(label + "/first", 16) if k % 5 == 0 else None  # (the two-block J0 hash)
        nonce, j0 = u.gcm_record(key, len(pt), case, label, first)
        ok, ct, tag = o.seal(o.AES_GCM, key, nonce, pt, b"ad")
        assert ok
        want = [o.aes_block(key, u.gcm_counter_block(j0, i)) for i in range(NB)]
        want[-1] = want[-1][:11]
        assert _keystream(ct, pt) == want, case
        assert o.open_(o.AES_GCM, key, nonce, ct, b"ad", tag) == (True, pt)
        if case[2] is not None:  # the edge lies inside the record
            assert int.from_bytes(j0[12:], "big") + 1 + case[2] == u.EDGE[case[0]]


@pytest.mark.parametrize("aead", list(u.SIV_KEYLEN))
def test_siv_keystream_follows_le32(aead):
    key = derive("edge-ref/" + aead, u.SIV_KEYLEN[aead])
    (cases,) = u.plan_row("siv", [NB] * len(u.all_cases("siv", LANES)), LANES, max_batches=1)
    assert {c[0] for c in cases} == set(u.SIV_CLASSES)
    for k, case in enumerate(cases):
        nonce, ad, pt, tag = u.siv_record(key, 16 * NB - 5, case, f"edge-ref/{aead}/{k}", k)
        assert int.from_bytes(tag[:4], "little") + case[2] == u.EDGE[case[0]]
        ok, ct, sealed = o.seal(o.AES_GCM_SIV, key, nonce, pt, ad)
        assert ok and sealed == tag
        _, enc = u.siv_record_keys(key, nonce)
        want = [o.aes_block(enc, u.siv_counter_block(tag, i)) for i in range(NB)]
        want[-1] = want[-1][:11]
        assert _keystream(ct, pt) == want, case
        assert o.open_(o.AES_GCM_SIV, key, nonce, ct, ad, tag) == (True, pt)


@pytest.mark.parametrize("aead", list(u.EAX_KEYLEN))
def test_eax_counter_carries(aead):
    key = derive("edge-ref/" + aead, u.EAX_KEYLEN[aead])
    nb = 40
    pt = u.data(2, 16 * nb - 5)
    cases = [(c, w, w) for c in u.EAX_CLASSES for w in (1, 17, nb - 2, nb - 1)]
    for k, case in enumerate(cases):
        nonce, n = u.eax_record(key, case, f"edge-ref/{aead}/{k}")
        assert ccm_eax_ref.eax_n(key, nonce) == n
        ct, tag = ccm_eax_ref.seal(aead, key, nonce, pt, b"ad")
        n_int = int.from_bytes(n, "big")
        want = [o.aes_block(key, ((n_int + i) % (1 << 128)).to_bytes(16, "big")) for i in range(nb)]
        want[-1] = want[-1][:11]
        assert _keystream(ct, pt) == want, case
        assert ccm_eax_ref.open_(aead, key, nonce, ct, b"ad", tag) == pt


# ---------------------------------------------------------------------------
# the reference library's records

def test_fixture_shape_and_inputs():
    fx = load("ref_ctr_edge.json")
    assert collections.Counter(r["aead"] for r in fx) == u.FIXTURE_COUNTS
    per_class = collections.Counter((r["aead"], r["class"]) for r in fx)
    for aead in u.GCM_KEYLEN:
        assert [per_class[aead, c] for c in u.GCM_CLASSES] == [5, 4, 4, 1, 1]
        assert sum(1 for r in fx if r["aead"] == aead and len(r["nonce"]) == 64) == 1
    for aead in u.SIV_KEYLEN:
        assert [per_class[aead, c] for c in u.SIV_CLASSES] == [2, 2, 2]
    for aead in u.EAX_KEYLEN:
        assert [per_class[aead, c] for c in u.EAX_CLASSES] == [2, 2, 2]
    # the committed inputs are the ones ctr_edge_util crafts
    ins = u.fixture_inputs()
    assert len(ins) == len(fx)
    for r, want in zip(fx, ins):
        assert (r["aead"], r["class"], r["w"]) == (want["aead"], want["class"], want["w"])
        assert all(bytes.fromhex(r[f]) == want[f] for f in ("key", "nonce", "ad", "pt"))
        assert len(want["pt"]) == u.FIXTURE_LEN <= 640


def test_oracle_and_restatement_match_reference_records():
    ids = {"gcm": o.AES_GCM, "siv": o.AES_GCM_SIV}
    for r in load("ref_ctr_edge.json"):
        key, nonce, ad, pt, ct, tag = (bytes.fromhex(r[f])
                                       for f in ("key", "nonce", "ad", "pt", "ct", "tag"))
        what = (r["aead"], r["class"], r["w"])
        if r["aead"].endswith("eax"):
            assert ccm_eax_ref.seal(r["aead"], key, nonce, pt, ad) == (ct, tag), what
            assert ccm_eax_ref.open_(r["aead"], key, nonce, ct, ad, tag) == pt, what
        else:
            aid = ids["siv" if r["aead"].endswith("siv") else "gcm"]
            assert o.seal(aid, key, nonce, pt, ad) == (True, ct, tag), what
            assert o.open_(aid, key, nonce, ct, ad, tag) == (True, pt), what
