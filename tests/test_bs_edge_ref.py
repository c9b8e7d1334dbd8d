"""The cases of test_bs_edge_gpu.py, checked on the CPU: that the length sets
put the partial block and the first empty slot at every (lane, slot) of the
table-free engine's chunks, that the planner (bs_edge_util.plan, a host
restatement of gcm_bs.hip bs_unit's nv / tl / statement choice) gives
hand-worked values, and that the CPU oracle at these lengths equals AES-GCM
restated block by block.  No GPU.
"""
import numpy as np
import pytest

import bs_edge_util as u
import oracle_lib as o


# ---------------------------------------------------------------------------
# 1. coverage

@pytest.mark.parametrize("L,count", [(2, 288), (8, 768), (16, 1536 + 18)])
def test_length_sets_reach_every_position(L, count):
    lens = u.set_lens(L)
    assert len(lens) == len(set(lens)) == count
    if L == 2:
        assert max(lens) < 4096
    if L == 8:
        assert min(lens) == 4096 and max(lens) <= 8191
    chunks = u.SET_CHUNKS[L]
    every = {(q, n) for q in range(L) for n in range(16)}
    for r in (0, 1, 15):
        # (r = 1, 15: the partial block; r = 0: the first empty slot)
        by_chunk = {c: set() for c in chunks}
        for x in lens:
            c, q, n = u.position(x, L)
            if x % 16 == r and c in by_chunk:
                by_chunk[c].add((q, n))
        assert by_chunk[chunks[0]] == every, (L, r, "first chunk")
        assert all(by_chunk[c] == every for c in chunks[1:]), (L, r, "later chunks")
    # The planner agrees: one record of r = 1 or 15 has its tail at that
    # position of its last chunk, and no other lane has one.
    for x in lens[1::3] + lens[2::3]:
        c, q, n = u.position(x, L)
        last = [p for p in u.plan([x], L)][-1]
        assert last[1] == c and last[4] == "tail"
        assert [(lane, t) for lane, t in enumerate(last[3]) if t >= 0] == [(q, n)], x
    # ... and one of r = 0 ends with nv = slot + (lane < q) full blocks.
    for x in lens[0::3]:
        c, q, n = u.position(x, L)
        ps = [p for p in u.plan([x], L)]
        assert all(t < 0 for p in ps for t in p[3])
        if (q, n) != (0, 0):
            assert ps[-1][1] == c and ps[-1][2][:L] == [n + (lane < q) for lane in range(L)], x
        else:
            assert len(ps) == c  # (a whole number of chunks: chunk c does not exist)


@pytest.mark.parametrize("L,lens", [(16, u.UNIFORM_16), (2, u.UNIFORM_2)])
def test_uniform_lists_reach_every_wave_uniform_nv(L, lens):
    cov = u.uniform_coverage(lens, L)
    assert cov["uniform_nv"] == set(range(17))
    assert cov["statements"] == {"full", "tail", "masked"}
    # The masked statement with a wave-uniform nv (whole memory instructions
    # with EXEC = 0): all of 1..15 in full units, without a tail.
    masked = {nv[0] for x in lens for _, _, nv, _, s in u.plan([x] * (64 // L), L)
              if s == "masked" and len(set(nv)) == 1}
    assert masked >= set(range(1, 16))


def test_uniform_8_lane_list():
    """Case 6: units of eight records of one long length."""
    got = set()
    for x in u.UNIFORM_8_LONG:
        assert 4096 <= x
        c, nv, tl, stmt = list(u.plan([x] * 8, 8))[-1][1:]
        k, r = (x - 6144) // 128, x % 128
        if (k, r) == (0, 0):
            assert (c, stmt) == (2, "full")
            continue
        assert c == 3 and stmt == ("tail" if r else "masked") and set(nv) == {k}
        got.add((k, stmt))
    assert got == {(0, "tail"), (1, "masked"), (1, "tail"), (8, "masked"), (8, "tail"),
                   (15, "masked"), (15, "tail")}


def test_unordered_batches_reach_everything():
    """The shuffles of cases 1, 7 and 8 as the GPU tests build them."""
    lens = u.shuffled(u.set_lens(16), len(u.set_lens(16)), 1)
    assert len(lens) < 4096
    u.assert_unordered_coverage(lens, 16)
    ki = [(i + i // 5) % 3 for i in range(len(lens))]
    u.assert_unordered_coverage(lens, 16, ("tail", "masked"), ki=ki)
    # TLS 1.3 records: the r = 0 and r = 15 members with one extra byte
    xt = [x for x in lens if x % 16 != 1]
    u.assert_unordered_coverage(xt, 16, xlen=1)


# ---------------------------------------------------------------------------
# 2. the planner against hand-worked cases

def test_planner_4097_at_16_lanes():
    """4,097 bytes: 256 full blocks and one byte.  Chunk 0 is full; in chunk 1
    block 256 is lane 0's slot 0."""
    ps = list(u.plan([4097] * 4, 16))
    assert [(p[0], p[1], p[4]) for p in ps] == [(0, 0, "full"), (0, 1, "tail")]
    assert ps[0][2] == [16] * 64 and ps[0][3] == [-1] * 64
    assert ps[1][2] == [0] * 64
    assert ps[1][3] == ([0] + [-1] * 15) * 4


def test_planner_1350_at_2_lanes():
    """1,350 bytes: 84 full blocks and 6 bytes, 85 blocks.  Chunks of 32:
    chunk 2 holds blocks 64..84, lane 0 the even ones (64..82: ten full, then
    block 84, the partial one, in slot 10), lane 1 the odd ones (65..83: ten)."""
    ps = list(u.plan([1350] * 32, 2))
    assert [(p[1], p[4]) for p in ps] == [(0, "full"), (1, "full"), (2, "tail")]
    assert ps[2][2] == [10, 10] * 32
    assert ps[2][3] == [10, -1] * 32


def test_planner_6528_at_8_lanes():
    """6,144 + 128 * 3 bytes: 408 blocks, chunks of 128: chunk 3 holds blocks
    384..407, three rows of eight."""
    ps = list(u.plan([6144 + 128 * 3] * 8, 8))
    assert [(p[1], p[4]) for p in ps] == [(0, "full"), (1, "full"), (2, "full"), (3, "masked")]
    assert ps[3][2] == [3] * 64 and ps[3][3] == [-1] * 64


def test_planner_dead_slots_and_extra_byte():
    """Three records in a unit of four (L = 16): the dead slot's lanes have
    nv = 0, so a chunk the live records fill is masked, not full.  An extra
    byte after a whole number of blocks is a block of its own: the tail."""
    ps = list(u.plan([4096] * 3, 16))
    assert [(p[1], p[4]) for p in ps] == [(0, "masked")]
    assert ps[0][2] == [16] * 48 + [0] * 16 and ps[0][3] == [-1] * 64
    ps = list(u.plan([32] * 32, 2, xlen=1))
    assert [(p[1], p[4]) for p in ps] == [(0, "tail")]
    assert ps[0][2] == [1, 1] * 32 and ps[0][3] == [1, -1] * 32
    # 47 bytes and the extra byte: the third block is complete, still the tail
    ps = list(u.plan([47] * 32, 2, xlen=1))
    assert ps[0][2] == [1, 1] * 32 and ps[0][3] == [1, -1] * 32
    # keyset: records 0 and 2 under key 0, record 1 under key 1, two passes
    ps = list(u.plan([4096, 4096, 4096], 16, ki=[0, 1, 0]))
    assert [(p[0], p[4]) for p in ps] == [((0, 0), "masked"), ((0, 1), "masked")]
    assert ps[0][2] == [16] * 16 + [0] * 16 + [16] * 16 + [0] * 16
    assert ps[1][2] == [0] * 16 + [16] * 16 + [0] * 32


# ---------------------------------------------------------------------------
# 3. the oracle at these lengths against AES-GCM block by block

@pytest.mark.parametrize("aead", ["aes-128-gcm", "aes-256-gcm"])
@pytest.mark.parametrize("L", [2, 8, 16])
def test_oracle_equals_blockwise_gcm(L, aead):
    rng = np.random.default_rng(100 + L)
    key = u.key_of(aead)
    for x in u.set_lens(L)[::7]:
        nonce = rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
        pt = rng.integers(0, 256, x, dtype=np.uint8).tobytes()
        ct = u.ctr_restated(key, nonce, pt)
        for ad_len in (0, 13, 16, 17, 16 * L + 1):
            ad = rng.integers(0, 256, ad_len, dtype=np.uint8).tobytes()
            ok, got_ct, got_tag = o.seal(o.AES_GCM, key, nonce, pt, ad)
            assert ok and got_ct == ct, (aead, x, ad_len)
            assert got_tag == u.ghash_tag_restated(key, nonce, ct, ad), (aead, x, ad_len)
