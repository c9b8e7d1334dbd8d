"""gcm_siv_kernel (gcm_siv.hip siv_record) against the CPU oracle at every
lane, block and unit edge, bit for bit.

siv_record deals POLYVAL's input [AD blocks, message blocks, length block] to
a record's 16 lanes and multiplies each lane's sum by H^e, e = n - jlast; a
wave runs units of four records, one per lane group.  The grid of
siv_edge_util (nA in [0, 17] and nP in [0, 33] blocks, last blocks of 16, 1
or 15 bytes: 5,200 records) puts every kind of block, every e, both partial
blocks and the length block on every lane, which the tests assert through the
planner (siv_edge_util.plan) per lane group before they launch.  The other
tests pick what the grid cannot: both memory paths of load_block / store_block
with `in`, `out`, `ad` and `tags` misaligned independently, units whose four
records diverge, dead records among live ones, a batch large enough that every
wave reuses its LDS slots under seven keys, every subset of the four layout
arrays, and iovec records cut at chosen points.

Every batch (siv_edge_util.run_batch / run_iov): seal equal to the oracle in
ciphertext, tag and status; then open untouched, with tag bit 127 of one
record flipped (the counter block has that bit forced, so only the 128-bit
compare can reject it) and with another record's last ciphertext byte
flipped -- every record's status, a failed record's len bytes zeroed and no
more, the pattern around every record and past the end of tags and status
intact after every launch, and the kernel's name.
"""
import itertools

import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import siv_edge_util as u  # noqa: E402

pytestmark = pytest.mark.gpu

AEADS = [u.A128, u.A256]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def grids():
    """The grid sealed by the oracle, once per key size; shared and left
    unchanged by the tests that run it or a part of it."""
    made = {}

    def get(aead):
        if aead not in made:
            made[aead] = u.Records(aead, u.grid())
        return made[aead]
    return get


# ---------------------------------------------------------------------------
# 1. the grid, in every lane group

@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("aead", AEADS)
def test_grid(grids, aead, k, inplace):
    """The whole grid as one ragged one-key batch, rotated by k records: grid
    record g sits at position (g + k) mod 5,200, so over k = 0..3 in each of
    the four lane groups; each rotation alone reaches everything in each."""
    R = grids(aead)
    order = u.rotated(range(R.n), k)
    u.assert_groups_reach_everything([R.geoms[g] for g in order], ("rotation", k))
    u.run_batch(R, order, route=f"grid/rot{k}", inplace=inplace)


# ---------------------------------------------------------------------------
# 2. alignment: the two memory paths of load_block and store_block

@pytest.mark.parametrize("mi,mo", [(0, 0), (0, 7), (9, 0), (3, 3)])
@pytest.mark.parametrize("aead", AEADS)
def test_alignment(grids, aead, mi, mo):
    """Every fifth grid record at byte-granular offsets (every off mod 16)
    with `in` at base + mi, `out` at + mo, `ad` at + 1 and `tags` at + 5: for
    `in` and for `out` some whole block goes by one uint4 and some by bytes."""
    R = grids(aead)
    order = list(range(0, R.n, 5))
    lens = [R.geoms[g][1] for g in order]
    offs, _ = u.ragged_offsets(lens, packed=True)
    assert {x % 16 for x in offs} == set(range(16))
    assert u.block_paths(mi, offs, lens) == u.block_paths(mo, offs, lens) == {"uint4", "bytes"}
    u.run_batch(R, order, route="alignment", mis=(mi, mo, 1, 5), packed=True)
    if mi == mo:
        u.run_batch(R, order, route="alignment", mis=(mi, mo, 1, 5), packed=True, inplace=True)


# ---------------------------------------------------------------------------
# 3. units whose records diverge, and the inactive tail

UNIT = [(0, 0), (272, 4113), (13, 40), (1, 1)]  # (the third one is dead)
COUNTS = (1, 2, 3, 4, 5, 47, 48, 49, 95, 97)


@pytest.fixture(scope="module")
def unit_records():
    made = {}

    def get(aead):
        if aead not in made:
            made[aead] = u.Records(aead, UNIT * 25, nkeys=2, ki=[(i // 4) % 2 for i in range(100)],
                                   label="units", unique=True)
        return made[aead]
    return get


@pytest.mark.parametrize("r", range(4))
@pytest.mark.parametrize("aead", AEADS)
def test_divergent_units(unit_records, aead, r):
    """Units of an empty record, one of 17 + 258 + 1 blocks, a dead one (key
    index past the set: active but not live) and a 1-byte one, each in lane
    group (position + r) mod 4; batches of 1..97 records: 1 to 3 inactive
    records in the last unit, and one, two and three workgroups."""
    R = unit_records(aead)
    for n in COUNTS:
        order = list(range(r, r + n))
        dead = {i: len(R.keys) for i, g in enumerate(order) if R.geoms[g] == UNIT[2]}
        assert n < 4 or dead
        u.run_batch(R, order, route=f"units/rot{r}/n{n}", dead=dead, keyset=True)


# ---------------------------------------------------------------------------
# 4. keyset

@pytest.mark.parametrize("aead", AEADS)
def test_keyset(aead):
    """Five keys, neighbouring records under different keys; one key index
    equal to num_keys and one of 0x7fffffff: status 0, zeroed output and tag,
    the neighbours exact."""
    geoms = u.grid()[3::11]
    ki = [(i + i // 5) % 5 for i in range(len(geoms))]
    assert all(a != b for a, b in zip(ki, ki[1:]))
    R = u.Records(aead, geoms, nkeys=5, ki=ki, label="keyset")
    dead = {R.n // 3 + 1: 5, 2 * R.n // 3 + 2: 0x7fffffff}
    assert {u.group(i)[1] for i in dead} == {(0, 1), (1, 0)} and all(geoms[i][1] for i in dead)
    u.run_batch(R, route="keyset")
    u.run_batch(R, route="keyset/bad-index", dead=dead)
    u.run_batch(R, route="keyset/bad-index", dead=dead, inplace=True)


# ---------------------------------------------------------------------------
# 5. every wave reuses its LDS slots

def test_certain_slot_reuse():
    """2 x 48 x CUs + 3 short records under seven keys: the grid is one
    workgroup per CU and a workgroup has 48 slots, so every wave runs a second
    unit in the slots of its first -- the round keys and the five Shoup tables
    of the next record and key replace the last one's."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 48 * cus + 3
    lens, ads = (0, 1, 16, 17, 48), (0, 13, 17)
    geoms = [(ads[i % 3], lens[i % 5]) for i in range(n)]
    ki = [(i + i // 4) % 7 for i in range(n)]
    assert n > 48 * cus and sum(m + 32 for _, m in geoms) < 2 << 20
    assert all(len({ki[i + j] for j in range(4)}) == 4 for i in range(0, n - 3, 4))
    R = u.Records(u.A256, geoms, nkeys=7, ki=ki, label="reuse", unique=True)
    u.run_batch(R, route="reuse")


# ---------------------------------------------------------------------------
# 6. the layout branch

ARRAYS = sorted(u.ALL_ARRAYS)
SUBSETS = [frozenset(c) for k in range(5) for c in itertools.combinations(ARRAYS, k)]


@pytest.mark.parametrize("aead", AEADS)
def test_layout_arrays(aead):
    """Nine records of one length and one AD length at uniform strides, given
    with each of the 16 subsets of {offsets, lengths, ad_offsets, ad_lengths}
    as arrays and the rest as scalars: identical bytes.  None present and one
    key is the kernel's separate uniform branch; none present with key_index
    is not."""
    assert len(SUBSETS) == 16 and SUBSETS[0] == frozenset() and SUBSETS[-1] == u.ALL_ARRAYS
    R = u.Records(aead, [(17, 33)] * 9, label="layout", unique=True)
    results = [u.run_batch(R, route=("layout", sorted(s)), uniform=True, present=s)
               for s in SUBSETS]
    for s, (ct, tags) in zip(SUBSETS, results):
        assert bool((ct == results[0][0]).all() and (tags == results[0][1]).all()), sorted(s)
    K = u.Records(aead, [(17, 33)] * 9, nkeys=3, ki=[i % 3 for i in range(9)], label="layout",
                  unique=True)
    for s in (frozenset(), u.ALL_ARRAYS):
        u.run_batch(K, route=("layout/keyset", sorted(s)), uniform=True, present=s)


# ---------------------------------------------------------------------------
# 7. iovec records

CORNERS = [(a, m) for a in (0, 257, 271, 272) for m in (0, 513, 527, 528)]
IOV_BASE = CORNERS + [(40, 4113), (17, 33)]


def iov_records():
    """64 records: the grid's corners, (40, 4113) and (17, 33) in turn; the
    zero-length pieces move with the record's index; every (17, 33) is cut
    into 1-byte pieces, AD and message."""
    geoms = [IOV_BASE[i % len(IOV_BASE)] for i in range(64)]
    variants = ["bytes" if g == (17, 33) else (i + i // len(IOV_BASE)) % 8
                for i, g in enumerate(geoms)]
    return geoms, variants


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("aead", AEADS)
def test_iovec(aead, inplace):
    """Messages cut at every one of 1, 15, 16, 17, 255, 256, 257 and len - 1
    inside them and ADs at 1, 15, 16, 17, zero-length pieces at the front, in
    the middle and at the end, one record in 1-byte pieces throughout; `in` at
    base + 3 and `out` at + 9 with pieces at every alignment.  A failed
    record's pieces are zeroed and the pattern around every piece stays."""
    geoms, variants = iov_records()
    assert {v for v in variants if v != "bytes"} == set(range(8)) and "bytes" in variants
    # every cut point is inside some record, and each placement of the
    # zero-length pieces meets the long record
    assert all(any(0 < c < m for _, m in geoms) for c in u.MSG_CUTS)
    assert len({v for g, v in zip(geoms, variants) if g == (40, 4113)}) >= 3
    R = u.Records(aead, geoms, label="iovec", unique=True)
    u.run_iov(R, range(R.n), variants, route="iovec", inplace=inplace)
