"""The cases of test_siv_edge_gpu.py, checked on the CPU: that the planner
(siv_edge_util.plan, a host restatement of how gcm_siv.hip siv_record deals
POLYVAL's input to 16 lanes) gives hand-worked values, that the grid puts
every kind of block, every record-end weight e, the partial AD block, the
partial message block and the length block on every lane and leaves every
number of lanes idle -- in every lane group of every rotation -- and that the
CPU oracle at these records equals RFC 8452 restated in Python (POLYVAL in its
own field, not through GHASH) and the reference library's own seals
(tests/golden/ref_siv_edge.json).  No GPU.
"""
import numpy as np
import pytest

import oracle_lib as o
import siv_edge_util as u
from golden_util import load

AD, MSG, LEN = u.AD, u.MSG, u.LEN


# ---------------------------------------------------------------------------
# 1. the planner against hand-worked records

def test_planner_empty_record():
    """(0, 0): the length block alone, on lane 0, times H^1."""
    p = u.plan(0, 0)
    assert (p.nA, p.nP, p.n) == (0, 0, 1)
    assert p.lanes[0] == u.Lane(((LEN, 0, 16),), 0, 1, False)
    assert all(ln == u.Lane((), None, None, True) for ln in p.lanes[1:])


def test_planner_one_trip_of_ad():
    """(240, 0): 15 AD blocks and the length block, one per lane, lane q
    times H^(16 - q): lane 0 is the only e = 16."""
    p = u.plan(16 * 15, 0)
    assert (p.nA, p.nP, p.n) == (15, 0, 16)
    for q in range(15):
        assert p.lanes[q] == u.Lane(((AD, q, 16),), q, 16 - q, False)
    assert p.lanes[15] == u.Lane(((LEN, 15, 16),), 15, 1, False)


def test_planner_message_returns_to_lane_0():
    """(256, 1): 16 AD blocks fill the first trip; the 1-byte message block is
    lane 0's second element and the length block lane 1's."""
    p = u.plan(16 * 16, 1)
    assert (p.nA, p.nP, p.n) == (16, 1, 18)
    assert p.lanes[0] == u.Lane(((AD, 0, 16), (MSG, 16, 1)), 16, 2, False)
    assert p.lanes[1] == u.Lane(((AD, 1, 16), (LEN, 17, 16)), 17, 1, False)
    for q in range(2, 16):
        assert p.lanes[q] == u.Lane(((AD, q, 16),), q, 18 - q, False)
    assert p.lanes[2].e == 16
    assert u.where_of((256, 1), 0) == (0, MSG)


def test_planner_33_elements():
    """(257, 240): 17 AD blocks (the last of 1 byte), 15 message blocks and
    the length block: lane 0 makes three trips and ends on the length block,
    lane q > 0 holds AD block q and message block q - 1."""
    p = u.plan(257, 240)
    assert (p.nA, p.nP, p.n) == (17, 15, 33)
    assert p.lanes[0] == u.Lane(((AD, 0, 16), (AD, 16, 1), (LEN, 32, 16)), 32, 1, False)
    for q in range(1, 16):
        assert p.lanes[q] == u.Lane(((AD, q, 16), (MSG, 16 + q, 16)), 16 + q, 17 - q, False)
    assert p.lanes[1].e == 16
    assert u.where_of((257, 240), 239) == (15, MSG)


def test_planner_partial_blocks_side_by_side():
    """(17, 1): the 1-byte AD block on lane 1 and the 1-byte message block on
    lane 2; (241, 1): the same lane one trip apart."""
    p = u.plan(17, 1)
    assert [ln.elems for ln in p.lanes[:4]] == [((AD, 0, 16),), ((AD, 1, 1),), ((MSG, 2, 1),),
                                                ((LEN, 3, 16),)]
    assert sum(ln.idle for ln in p.lanes) == 12
    p = u.plan(16 * 15 + 1, 16 * 15 + 1)
    assert p.lanes[15].elems == ((AD, 15, 1), (MSG, 31, 1))


def test_lane_groups():
    assert [u.group(i) for i in (0, 1, 2, 3, 4, 7)] == [
        (0, (0, 0)), (0, (0, 1)), (0, (1, 0)), (0, (1, 1)), (1, (0, 0)), (1, (1, 1))]


# ---------------------------------------------------------------------------
# 2. coverage

def test_grid_shape():
    g = u.grid()
    assert len(g) == len(set(g)) == 52 * 100
    assert max(m for _, m in g) == 528 and max(a for a, _ in g) == 272
    assert {u.plan(a, m).nA for a, m in g} == set(range(18))
    assert {u.plan(a, m).nP for a, m in g} == set(range(34))
    assert {(a % 16, m % 16) for a, m in g} == {(x, y) for x in (0, 1, 15) for y in (0, 1, 15)}
    assert len(u.fixture_geoms()) == 81 and set(u.fixture_geoms()) <= set(g)


def test_grid_reaches_everything():
    u.assert_reaches_everything(u.coverage(u.grid()), "grid")


@pytest.mark.parametrize("k", range(4))
def test_grid_reaches_everything_in_every_lane_group(k):
    """Each rotation alone puts everything into each of the four lane groups
    (15 idle lanes, which only the record (0, 0) has, into the group it sits
    in); over the four rotations every geometry sits in every group."""
    recs = u.rotated(u.grid(), k)
    u.assert_groups_reach_everything(recs, ("rotation", k))
    assert recs[k] == u.grid()[0] == (0, 0) and u.group(k)[1] == u.GROUPS[k]
    assert len(recs) % 4 == 0  # (so record g sits in group (g + k) mod 4)


def test_partial_blocks_meet():
    """The partial AD block and the partial message block in neighbouring
    lanes, and in the same lane one trip apart, on every lane."""
    side, same = set(), set()
    for a, m in u.grid():
        p = u.plan(a, m)
        part = [(q, k, j) for q, ln in enumerate(p.lanes) for k, j, nb in ln.elems if nb < 16]
        pa = [(q, j) for q, k, j in part if k == AD]
        pm = [(q, j) for q, k, j in part if k == MSG]
        if pa and pm:
            (qa, ja), (qm, jm) = pa[0], pm[0]
            if jm == ja + 1:
                side.add(qa)
            if jm == ja + 16:
                same.add(qa)
    assert side == set(range(16)) and same == set(range(16))


def test_every_fifth_record_packed_takes_both_memory_paths():
    """The alignment batch: every off mod 16, and for each of the four base
    misalignments of `in` and `out` some whole block on the uint4 path and
    some on the bytewise one."""
    geoms = u.grid()[::5]
    lens = [m for _, m in geoms]
    offs, size = u.ragged_offsets(lens, packed=True)
    assert {x % 16 for x in offs} == set(range(16))
    for i in range(len(offs) - 1):
        assert offs[i] + lens[i] + u.GUARD <= offs[i + 1]
    assert offs[0] >= u.GUARD and offs[-1] + lens[-1] + u.GUARD <= size
    for base in (0, 3, 7, 9):
        assert u.block_paths(base, offs, lens) == {"uint4", "bytes"}
    # (aligned offsets on an aligned base never leave the uint4 path)
    assert u.block_paths(0, u.ragged_offsets(lens)[0], lens) == {"uint4"}


def test_guards_bite():
    """The comparison the GPU runners use reports a write one byte past a
    failed record's len -- shown by comparing against an expectation that is
    itself one byte too long -- and passes the exact one."""
    geoms = [(0, 1), (13, 16), (16, 31)]
    lens = [m for _, m in geoms]
    for packed in (False, True):
        offs, size = u.ragged_offsets(lens, packed)
        exact = u.arena_of(size, offs, [bytes(x) for x in lens])
        assert u.compare_arena(exact, exact.copy(), offs, lens, geoms) == ([], False)
        for i in range(3):
            long_ = exact.copy()
            long_[offs[i] + lens[i]] = 0  # an expected length of len + 1
            assert u.compare_arena(exact, long_, offs, lens, geoms) == ([], True)
            assert u.compare_arena(long_, exact, offs, lens, geoms) == ([], True)
            short = exact.copy()
            short[offs[i] + lens[i] - 1] = u.FILL  # a zero-fill that stops one byte early
            assert u.compare_arena(short, exact, offs, lens, geoms) == \
                ([(i, geoms[i], u.where_of(geoms[i], lens[i] - 1))], False)
    want = np.zeros(48, np.uint8)
    got = want.copy()
    got[16 + 15] = 0x80
    assert u.compare_tags(got, want, geoms) == [(1, (13, 16), u.lane_e((13, 16)))]
    assert u.lane_e((13, 16)) == [3, 2, 1] + [None] * 13


def test_open_variants():
    assert u.open_variants([0], [0]) == [("untouched", None, None), ("tag bit 127", 0, None)]
    v = u.open_variants([5, 0, 7, 9], [0, 2, 3])
    assert v[1][1] == 2 and v[2][2] in (0, 3) and len(v) == 3


def test_iov_pieces():
    R = u.Records(u.A128, [(40, 4113), (17, 33), (0, 0)], label="ref-pieces")
    parts, ad_parts = u.iov_pieces(R, 0, 7)
    assert b"".join(parts) == R.pt[0] and b"".join(ad_parts) == R.ad[0]
    assert [len(p) for p in parts] == [0, 1, 14, 1, 1, 238, 0, 1, 1, 3855, 1, 0]
    assert [len(p) for p in ad_parts] == [0, 1, 14, 1, 0, 1, 23]
    parts, ad_parts = u.iov_pieces(R, 1, "bytes")
    assert [len(p) for p in parts] == [1] * 33 and [len(p) for p in ad_parts] == [1] * 17
    assert u.iov_pieces(R, 2, 0) == ([b""], [b""])


# ---------------------------------------------------------------------------
# 3. the oracle against RFC 8452 restated, and both against the reference's seals

def test_polyval_field():
    """x^-128 is what RFC 8452 says it is, and POLYVAL matches the RFC's
    appendix A example."""
    assert u.clmul_mod(u.clmul_mod(1 << 127, 2), u.X_INV_128) == 1  # x^128 x^-128
    h = bytes.fromhex("25629347589242761d31f826ba4b757b")
    x = bytes.fromhex("4f4f95668c83dfb6401762bb2d01a262" "d1a24ddd2721d006bbe45f20d3c9f362")
    assert u.polyval(h, x).hex() == "f7a3b47b846119fae5b7866cf5e5b77e"


@pytest.mark.parametrize("aead", list(u.KEYLEN))
def test_oracle_equals_rfc8452_restated(aead):
    """Every seventh grid record: seal equal to the restatement, and open
    rejecting tag bit 127, the last ciphertext byte and the last AD byte."""
    key = u.key_of(aead)
    for a, m in u.grid()[::7]:
        nonce, ad, pt = u.record_data(a, m, "ref/" + aead)
        ok, ct, tag = o.seal(o.AES_GCM_SIV, key, nonce, pt, ad)
        assert ok and (ct, tag) == u.siv_seal_restated(key, nonce, pt, ad), (aead, a, m)
        assert o.open_(o.AES_GCM_SIV, key, nonce, ct, ad, tag) == (True, pt), (aead, a, m)
        flipped = tag[:15] + bytes([tag[15] ^ 0x80])
        assert not o.open_(o.AES_GCM_SIV, key, nonce, ct, ad, flipped)[0], (aead, a, m)
        if m:
            bad = ct[:-1] + bytes([ct[-1] ^ 1])
            assert not o.open_(o.AES_GCM_SIV, key, nonce, bad, ad, tag)[0], (aead, a, m)
        if a:
            bad = ad[:-1] + bytes([ad[-1] ^ 1])
            assert not o.open_(o.AES_GCM_SIV, key, nonce, ct, bad, tag)[0], (aead, a, m)


def test_restated_open_rejects_tag_bit_127():
    """Bit 127 of the tag leaves the counter block, so the keystream and
    POLYVAL's input, as they are: only the comparison sees it."""
    key = u.key_of(u.A128)
    nonce, ad, pt = u.record_data(17, 33, "ref/bit127")
    ct, tag = u.siv_seal_restated(key, nonce, pt, ad)
    flipped = tag[:15] + bytes([tag[15] ^ 0x80])
    assert u.siv_open_restated(key, nonce, ct, ad, tag) == (True, pt)
    assert u.siv_open_restated(key, nonce, ct, ad, flipped) == (False, pt)


def test_reference_fixture():
    """The reference library's seals of the fixture records equal the oracle's
    and the restatement's."""
    doc = load("ref_siv_edge.json")
    inputs = u.fixture_inputs()
    assert len(doc) == len(inputs) == 162
    for d, r in zip(doc, inputs):
        assert (d["aead"], d["ad_len"], d["len"]) == (r["aead"], r["ad_len"], r["len"])
        for f in ("key", "nonce", "ad", "pt"):
            assert bytes.fromhex(d[f]) == r[f], (d["aead"], d["ad_len"], d["len"], f)
        want = (bytes.fromhex(d["ct"]), bytes.fromhex(d["tag"]))
        what = (d["aead"], d["ad_len"], d["len"])
        assert o.seal(o.AES_GCM_SIV, r["key"], r["nonce"], r["pt"], r["ad"]) == (True,) + want, what
        assert u.siv_seal_restated(r["key"], r["nonce"], r["pt"], r["ad"]) == want, what
