"""The table-free AES-GCM engine (gcm_bs.hip bs_unit and the statements of
gcm_bs_io.inc) against the CPU oracle at every lane, slot and chunk edge, bit
for bit.

A record's blocks are dealt to L lanes in chunks of 16 L blocks; per chunk and
lane the kernel computes nv (full blocks, a prefix of the lane's 16 slots) and
tl (the slot of its partial or extra-byte block), and a wave ballot picks the
`full`, `tail` or masked statement.  The length sets of bs_edge_util put the
partial block (r = 1, 15) and the first empty slot (r = 0) at every one of the
16 L positions, in the first chunk and in a later one, on every route of
launch_gcm_bs:

    L = 16  one key, ragged, fewer than 4,096 records; uniform records of
            4 KiB or more; the keyset kernel; iovec records; the bitsliced
            waves of the mixed engine
    L = 8   the long class (4 KiB or more) of a length-ordered ragged batch
    L = 2   its short class; uniform records below 4 KiB

each also with the TLS 1.3 extra byte (XT) where the launcher has it, and with
the batched E_K(J0) production switched off (self_ek0).  Every test asserts
the launcher's predicates for the route it means (bs_edge_util.bs_lanes) and
the kernel's name; every batch that is not length-ordered also asserts, per
the planner (bs_edge_util.plan), which statements and (lane, slot) tails it
reaches.

Seal: ciphertext, tags and status equal the oracle's.  Open: of the sealed
batch with one record's tag and another's last ciphertext byte flipped; those
two get status 0 and zeroed output, the others their plaintext.  The space
around the records (16 bytes or more after each) holds a pattern that must
come back untouched.
"""
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import bs_edge_util as u  # noqa: E402
import oracle_lib as o  # noqa: E402
from test_gpu_parity import IovArena  # noqa: E402

pytestmark = pytest.mark.gpu

A128, A192, A256 = "aes-128-gcm", "aes-192-gcm", "aes-256-gcm"
LENS16, LENS8, LENS2 = u.set_lens(16), u.set_lens(8), u.set_lens(2)
N_SPLIT = 4224  # >= 4,099: four cycles of the 768 + 288 lengths


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


@pytest.fixture
def bs(aes_engine):
    aes_engine("bs")


@pytest.fixture
def no_ek0_producers():
    prev = ba.test_set_bs_ek0_producers(False)
    yield
    ba.test_set_bs_ek0_producers(prev)


def batch_16():
    """Case 1's batch: every length of the L = 16 set once, shuffled."""
    lens = u.shuffled(LENS16, len(LENS16), 1)
    assert sorted(lens) == sorted(LENS16) and len(lens) < 4096
    return lens


def batch_split(n=N_SPLIT):
    """Case 2's batch: the L = 8 and L = 2 sets cycled, shuffled."""
    lens = u.shuffled(LENS8 + LENS2, n, 2)
    assert n >= 4099  # (wants_length_order)
    long_, short = [x for x in lens if x >= 4096], [x for x in lens if x < 4096]
    assert long_ and short and set(long_) == set(LENS8) and set(short) == set(LENS2)
    return lens


# ---------------------------------------------------------------------------
# one key

@pytest.mark.parametrize("aead,odd", [(A128, 0), (A128, 3), (A256, 0), (A256, 3)])
def test_ragged_16_lanes(bs, aead, odd):
    """1. All 1,536 + 18 lengths once: all three statements, and a tail at
    every (lane, slot).  Offsets 16-byte aligned, or 3 mod 16 (the byte path)."""
    lens = batch_16()
    u.assert_unordered_coverage(lens, 16)
    u.check_ragged(aead, lens, lanes=(16,), route="ragged-16", odd=odd)


def test_ragged_16_lanes_aes192(bs):
    """1. AES-192 on every fifth length."""
    lens = batch_16()[::5]
    cov = u.coverage(u.plan(lens, 16), 16)
    assert cov["statements"] == {"full", "tail", "masked"}
    u.check_ragged(A192, lens, lanes=(16,), route="ragged-16/192")


@pytest.mark.parametrize("aead", [A128, A256])
def test_length_ordered_split(bs, aead):
    """2. The long class at 8 lanes and the short one at 2, each in length
    order: every length of both sets."""
    u.check_ragged(aead, batch_split(), lanes=(8, 2), route="split-8-2")


@pytest.mark.parametrize("batch", ["ragged-16", "split-8-4"])
def test_table_engine_control(aes_engine, batch):
    """3. The same two ragged batches under the T-table engine (gcm_kernel at
    16 lanes, and at 8 and 4 in length order): its tail lanes at every lane."""
    aes_engine("table")
    # (`lanes` names the length classes, whose predicates both engines share:
    # failures are located as the table-free engine would deal the blocks)
    if batch == "ragged-16":
        u.check_ragged(A128, batch_16(), lanes=(16,), route=batch, kernel="gcm_kernel")
    else:
        u.check_ragged(A128, batch_split(), lanes=(8, 2), route=batch, kernel="gcm_kernel")


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("k", range(16))
def test_uniform_16_lanes(bs, k, inplace):
    """4. 4,096 + 256 k + r bytes: in chunk 1 every lane has nv = k (r = 0:
    the masked statement with whole memory instructions under EXEC = 0; r = 1:
    the same with lane 0's tail), k + 1 in lane 0 (r = 17), or k + 1 in
    lanes 0..14 with the tail in lane 15 (r = 255).  67 records: the last
    unit has a dead record."""
    for r in (0, 1, 17, 255):
        rlen = 4096 + 256 * k + r
        assert rlen in u.UNIFORM_16
        u.check_uniform(A128, rlen, lanes=(16,), route="uniform-16", inplace=inplace)


def test_uniform_16_lanes_two_chunks(bs):
    """4. 8,192 bytes: two full chunks."""
    assert [p[4] for p in u.plan([8192] * 4, 16)] == ["full", "full"]
    u.check_uniform(A128, 8192, lanes=(16,), route="uniform-16")
    u.check_uniform(A128, 8192, lanes=(16,), route="uniform-16", inplace=True)


@pytest.mark.parametrize("c", [0, 2])
def test_uniform_2_lanes(bs, c):
    """5. 512 c + 32 k + r bytes, length 0 included: two full units of 32
    records and one with three live ones."""
    for k in range(16):
        for r in (0, 1, 17, 31):
            rlen = 512 * c + 32 * k + r
            assert rlen in u.UNIFORM_2
            u.check_uniform(A128, rlen, lanes=(2,), route="uniform-2", inplace=(k + r) % 2 == 1)


@pytest.mark.parametrize("rlen", u.UNIFORM_8_LONG)
def test_wave_uniform_8_lanes(bs, rlen):
    """6. A length-ordered batch of 4,100 records with one long length (523
    records: 65 whole units of eight and one of three) and one short one."""
    lens = [rlen] * 523 + [u.UNIFORM_8_SHORT] * (4100 - 523)
    random.Random(rlen).shuffle(lens)
    u.check_ragged(A128, lens, lanes=(8, 2), route="split-8-2/uniform", seed=rlen)


# ---------------------------------------------------------------------------
# the other kernels that instantiate bs_unit

def keys_of(n):
    return [(i + i // 5) % 3 for i in range(n)]


def test_keyset_16_lanes(bs):
    """7. Case 1's batch under three keys: every tile runs three passes with
    inactive groups (no unit holds one key only, so no chunk is `full`).  One
    record carries a key index past the key set."""
    lens = batch_16()
    ki = keys_of(len(lens))
    assert all(set(ki[t:t + 64]) == {0, 1, 2} for t in range(0, len(lens), 64))
    u.assert_unordered_coverage(lens, 16, ("tail", "masked"), ki=ki)
    u.check_ragged(A128, lens, lanes=(16,), route="keyset", ki=ki, nkeys=3)
    dead = len(lens) // 2 + 1
    ki[dead] = 3
    u.check_ragged(A128, lens, lanes=(16,), route="keyset/bad-index", ki=ki, nkeys=3, dead=(dead,))


def xt_lens(lens):
    """The r = 0 members (the extra byte is a block of its own: nb = nfull + 1)
    and the r = 15 ones (it completes a block that is still the tail)."""
    return [x for x in lens if x % 16 in (0, 15)]


def test_tls13_ragged_16_lanes(bs):
    """8. TLS 1.3 records, ragged, fewer than 4,096."""
    lens = u.shuffled(xt_lens(LENS16), len(xt_lens(LENS16)), 8)
    u.assert_unordered_coverage(lens, 16, xlen=1)
    u.check_tls13(lens, lanes=(16,), route="tls13-ragged-16")


def test_tls13_uniform_2_lanes(bs):
    """8. TLS 1.3 records, uniform and short: every slot of both lanes in
    chunk 0, and chunk 1's first and last."""
    lens = xt_lens(u.edge_lens(2, (0,)) + u.edge_lens(2, (1,), (0, 1, 30, 31)))
    tails = set()
    for rlen in lens:
        p = list(u.plan([rlen] * 32, 2, xlen=1))[-1]
        assert p[4] == "tail"
        tails |= {(p[1], lane % 2, t) for lane, t in enumerate(p[3]) if t >= 0}
        u.check_tls13([rlen] * u.N_UNIFORM, lanes=(2,), route="tls13-uniform-2", uniform=True,
                      seed=rlen)
    assert tails >= {(0, q, n) for q in range(2) for n in range(16)}


def test_tls13_length_ordered_split(bs):
    """8. TLS 1.3 records, 4,224 ragged ones: 8 and 2 lanes."""
    lens = u.shuffled(xt_lens(LENS8 + LENS2), N_SPLIT, 9)
    assert set(lens) == set(xt_lens(LENS8 + LENS2)) and len(lens) >= 4099
    u.check_tls13(lens, lanes=(8, 2), route="tls13-split-8-2")


def test_iovec_16_lanes(bs):
    """9. Every fifth length of the L = 16 set as iovec records, cut at
    256 m + d for every run boundary m = 1..15 of the first chunk and d in
    {-1, 0, 1}: a zero-length piece, then a 1-byte piece next to the cut,
    then the rest; records by turns in place and not.  bs_iov_slow is entered
    at, beside and away from the boundaries of a chunk's runs."""
    aead, key = A128, u.key_of(A128)
    lens = u.shuffled(LENS16[::5], len(LENS16[::5]), 10)
    n = len(lens)
    assert u.bs_lanes(n, True, 0, iov=True) == (16,)
    rng = random.Random(11)
    pts = [rng.randbytes(x) for x in lens]
    ads = [rng.randbytes((0, 13, 16, 17, 40)[i % 5]) for i in range(n)]
    nonces = [rng.randbytes(12) for _ in range(n)]
    cuts_seen = set()
    chunks, starts, ad_chunks, ad_starts = [], [0], [], [0]
    pos, apos = 16, 0
    for i in range(n):
        m, d = 1 + i % 15, (-1, 0, 1)[(i // 15) % 3]
        cut = 256 * m + d
        x, in_place = lens[i], i % 2 == 1
        if cut + 1 < x:
            pieces = [pts[i][:cut], b"", pts[i][cut:cut + 1], pts[i][cut + 1:]]
            cuts_seen.add((m, d))
        else:
            pieces = [pts[i][:x // 2], b"", pts[i][x // 2:]]
        assert b"".join(pieces) == pts[i]
        for part in pieces:
            pos += 16 + rng.randint(0, 7)  # (a gap of pattern after every piece)
            chunks.append((pos, part, in_place))
            pos += len(part)
        starts.append(len(chunks))
        apos += rng.randint(0, 3)
        ad_chunks.append((apos, ads[i]))
        apos += len(ads[i])
        ad_starts.append(len(ad_chunks))
    assert cuts_seen == {(m, d) for m in range(1, 16) for d in (-1, 0, 1)}
    arena = IovArena(chunks, starts, ad_chunks, ad_starts, nonces)
    in_src = np.zeros(arena.d_src.numel(), bool)
    for off, part, _ in chunks:
        in_src[off:off + len(part)] = True
    src = arena.d_src.cpu().numpy()
    src[~in_src] = u.FILL
    arena.d_src.copy_(torch.from_numpy(src))
    arena.d_dst.fill_(u.FILL)
    src_before = arena.d_src.cpu().numpy()
    ctx = ba.AEADCtx(aead, key, 16)
    res = []
    u.timed(lambda: res.append(arena.seal(ctx)), "gcm_bs_kernel")
    cts, tags, st = res[0]
    want = [o.seal(o.AES_GCM, key, nonces[i], pts[i], ads[i]) for i in range(n)]
    bad = [(i, lens[i]) for i in range(n)
           if (True, cts[i], tags[16 * i:16 * i + 16].tobytes()) != want[i]]
    assert bad == [] and st.tolist() == [1] * n, ("iovec seal: [(record, length)]", bad)
    # Outside the pieces written, both arenas are as they were.
    src_after, dst_after = arena.d_src.cpu().numpy(), arena.d_dst.cpu().numpy()
    w_src, w_dst = np.zeros(src_after.size, bool), np.zeros(dst_after.size, bool)
    for off, part, in_place in chunks:
        (w_src if in_place else w_dst)[off:off + len(part)] = True
    assert np.array_equal(src_after[~w_src], src_before[~w_src])
    assert (dst_after[~w_dst] == u.FILL).all()
    # Open with every seventh tag and one record's last byte damaged.
    damaged = set(range(0, n, 7))
    tg = tags.copy()
    for i in damaged:
        tg[16 * i + i % 16] ^= 1
    last = next(i for i in range(n // 2, n) if i not in damaged and lens[i] % 16 == 1)
    arena.flip_ciphertext_bit(last, lens[last] - 1, 4)
    damaged.add(last)
    res = []
    u.timed(lambda: res.append(arena.open(ctx, tg)), "gcm_bs_kernel")
    back, st = res[0]
    bad = [(i, lens[i]) for i in range(n)
           if (st[i], back[i]) != ((0, bytes(lens[i])) if i in damaged else (1, pts[i]))]
    assert bad == [], ("iovec open: [(record, length)]", bad)


@pytest.fixture
def mix4():
    prev = ba.test_set_gcm_mix(4)
    yield
    ba.set_aes_gcm_engine(prev)


@pytest.mark.parametrize("rlen", u.MIX_LENS)
def test_mixed_engine(mix4, rlen):
    """10. The mixed engine with four bitsliced waves: 257 records are 65
    units on one counter for 16 waves, so both wave roles take units."""
    assert rlen in u.UNIFORM_16
    # (gcm_mix_eligible: AES-128, one key, uniform, no AD arrays, 4 KiB or more)
    assert rlen >= 4096 and u.N_MIX > 1
    u.check_uniform(A128, rlen, n=u.N_MIX, lanes=(16,), route="mix4", kernel="gcm_mix_kernel")


def test_self_ek0_ragged_16_lanes(bs, no_ek0_producers):
    """11. Case 1's batch with the E_K(J0) producers off: every record end
    computes its own."""
    u.check_ragged(A128, batch_16(), lanes=(16,), route="ragged-16/self_ek0")


def test_self_ek0_length_ordered_split(bs, no_ek0_producers):
    """11. Case 2's batch likewise."""
    u.check_ragged(A128, batch_split(), lanes=(8, 2), route="split-8-2/self_ek0")


# ---------------------------------------------------------------------------
# AD and batch-count edges

def ad_cycle(n, lanes):
    """n AD lengths cycling 16 m + s, m around L and 2 L for every L of the
    route, shifted per unit of 64 records."""
    lens = sorted({x for L in lanes for x in u.ad_fold_lens(L)})
    return [lens[(i + i // 64) % len(lens)] for i in range(n)], lens


@pytest.mark.parametrize("route", ["ragged-16", "split-8-2", "uniform-2", "keyset"])
def test_ad_fold(bs, route):
    """12. record_ad_hash<L>: per-record AD lengths of 16 m + s bytes, m in
    {0, 1, 2, L - 1, L, L + 1, 2 L, 2 L + 1}, s in {0, 1, 15}; record lengths
    every ninth member of the route's set."""
    if route in ("ragged-16", "keyset"):
        lens = u.shuffled(LENS16[::9], 2 * len(LENS16[::9]), 12)
        ads, every = ad_cycle(len(lens), (16,))
        assert set(ads) == set(every)
        kw = dict(ki=keys_of(len(lens)), nkeys=3) if route == "keyset" else {}
        u.check_ragged(A128, lens, lanes=(16,), route="ad/" + route, ad_lens=ads, **kw)
    elif route == "split-8-2":
        lens = u.shuffled(LENS8[::9] + LENS2[::9], 4099, 13)
        ads, every = ad_cycle(len(lens), (8, 2))
        for cls in (True, False):  # every AD length in both classes
            assert {a for x, a in zip(lens, ads) if (x >= 4096) == cls} == set(every)
        u.check_ragged(A128, lens, lanes=(8, 2), route="ad/" + route, ad_lens=ads)
    else:
        ads, every = ad_cycle(u.N_UNIFORM, (2,))
        assert set(ads) == set(every)
        for rlen in LENS2[::9]:
            u.check_uniform(A128, rlen, lanes=(2,), route="ad/" + route, ad_lens=ads)


@pytest.mark.parametrize("L,rlen", [(2, 1350), (16, 4097)])
def test_ad_fold_uniform_ad(bs, L, rlen):
    """12. One AD length for the whole batch: 0 and 16 (many_ad false in every
    wave), 17 and 16 L + 1 (true in every wave)."""
    for ad_len in (0, 16, 17, 16 * L + 1):
        u.check_uniform(A128, rlen, lanes=(L,), route=f"ad-uniform-{L}", ad_lens=ad_len)


@pytest.mark.parametrize("layout", ["uniform-2", "keyset"])
def test_batch_counts(bs, layout):
    """13. Batch counts around the E_K(J0) groups of 1,024 positions (produced
    by units 0..3 and each group's middle unit): uniform 40-byte records at 2
    lanes, and 48-byte records under two keys.  Parity cannot tell a missing
    producer from the bounded-poll fallback -- either way the record end has
    the right E_K(J0) -- so this checks the results at these counts, not which
    of the two delivered them."""
    for n in u.COUNTS:
        counts(layout, n)


@pytest.mark.parametrize("layout", ["uniform-2", "keyset"])
def test_batch_counts_self_ek0(bs, no_ek0_producers, layout):
    """13. With the producers off."""
    for n in u.COUNTS_NO_PRODUCERS:
        counts(layout, n)


def counts(layout, n):
    if layout == "uniform-2":
        u.check_uniform(A128, 40, n=n, lanes=(2,), route=f"counts/{n}")
    else:
        u.check_uniform(A128, 48, n=n, lanes=(16,), route=f"counts-keyset/{n}",
                        ki=[(i + i // 3) % 2 for i in range(n)], nkeys=2)
