"""The ChaCha20-Poly1305 kernels (chacha.hip) against the CPU oracle at every
block, unit and chunk edge, bit for bit.

launch_chacha routes a batch to one of six chacha_poly_kernel variants or to
chacha_one_kernel; the kernel-name hook reports them all under one name, so
every test asserts the launcher's own predicates on the layout it built
(buffer addresses mod 128, stride mod 128 and mod 16, offsets or none):

    lines   uniform, 128 | stride, buffers 128-byte aligned   COAL (sh = 1)
    quads   uniform, 16 | stride, 128 not dividing it          plain (sh = 0)
    any     uniform, base 1, stride not 16 k                   ANY
    ragged  offsets and lengths                                plain, aligned
                                                               or byte path
    TLS 1.3 records (one extra byte), ragged / lines           XT / XT + COAL
    iovec records                                              IOV
    one host record up to 16 KiB and 2,048 Poly1305 blocks     chacha_one_kernel

Lengths 64 k + r (chacha_edge_util.LENS) put every count of ChaCha blocks
under both lane parities in front of every residue of the last block; AD of
0..5 blocks; contents of all-0xff and all-zero ciphertext; and records solved
so that the Poly1305 accumulator ends at p - 1, 2^128, the all-zero tag, ...

Seal: ciphertext, tags and status equal the oracle's.  Open: of the sealed
batch with one record's tag and another's last ciphertext byte flipped; those
two get status 0 and zeroed output, the others their plaintext.  The space
between and around the records holds a pattern that must come back untouched.
"""
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import chacha_edge_util as u  # noqa: E402
import oracle_lib as o  # noqa: E402
import tls_util  # noqa: E402
from test_gpu_parity import DEV, IovArena, _t  # noqa: E402

pytestmark = pytest.mark.gpu

N = 67          # uniform: two full 32-record waves and one with three live records
N_RAGGED = 192
FILL = 0x5a
CHACHA = "chacha20-poly1305"
# Address of the first record modulo 128, by route.
BASE = {"lines": 0, "quads": 16, "any": 1, "ragged": 0}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


def dev_arena(host, base):
    """`host` on the device at an address = base mod 128, inside an allocation
    that holds the pattern on both sides.  Returns (allocation, view)."""
    whole = torch.full((len(host) + 256,), FILL, dtype=torch.uint8, device=DEV)
    lo = (base - whole.data_ptr()) % 128
    view = whole[lo:lo + len(host)]
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 128 == base
    return whole, view


def arena_out(whole, view):
    """The view's bytes, and whether the allocation around it kept the pattern."""
    w = whole.cpu().numpy()
    lo = view.data_ptr() - whole.data_ptr()
    margin = np.concatenate([w[:lo], w[lo + view.numel():]])
    return w[lo:lo + view.numel()], bool((margin == FILL).all())


def assert_route(route, d_in, d_out, stride):
    """launch_chacha's predicates (whole_lines, unaligned_uniform) for a
    batch without extra bytes."""
    ptrs = d_in.data_ptr() | d_out.data_ptr()
    if route == "lines":
        assert stride % 128 == 0 and ptrs % 128 == 0
    elif route == "quads":
        assert stride % 16 == 0 and stride % 128 != 0 and ptrs % 16 == 0
    elif route == "any":
        assert (ptrs | stride) % 16 != 0
    else:
        assert route == "ragged" and stride is None


def check(aead, keys, pts, ads, nonces, offs, size, route, *, ki=None, stride=None, inplace=False,
          expect=None):
    """Seal and open one batch: record i = pts[i] at offs[i] of an arena of
    `size` bytes, with AD ads[i] and nonce nonces[i].  `stride`: a uniform
    batch (no per-record arrays; one record length, one AD length).
    `expect` = (cts, tags) the oracle must produce (solved records)."""
    n = len(pts)
    lens, nl = [len(p) for p in pts], u.NONCE_LEN[aead]
    inside = np.zeros(size, bool)
    pt = np.full(size, FILL, np.uint8)
    for i in range(n):
        assert offs[i] + lens[i] <= size and not inside[offs[i]:offs[i] + lens[i]].any()
        pt[offs[i]:offs[i] + lens[i]] = np.frombuffer(pts[i], np.uint8)
        inside[offs[i]:offs[i] + lens[i]] = True
    lens64, offs64 = np.asarray(lens, np.uint64), np.asarray(offs, np.uint64)
    nonce_arr = np.frombuffer(b"".join(nonces), np.uint8).copy()
    assert nonce_arr.size == nl * n
    ad_lens = np.array([len(a) for a in ads], np.uint64)
    ad_offs = np.concatenate([[0], np.cumsum(ad_lens)[:-1]]).astype(np.uint64)
    ad_arr = np.frombuffer(b"".join(ads) + bytes([FILL]) * 16, np.uint8).copy()
    karr = np.frombuffer(b"".join(keys), np.uint8).copy()
    kidx = None if ki is None else np.asarray(ki, np.uint32)
    ref = np.full(size, FILL, np.uint8)
    ref_tags = np.zeros(16 * n, np.uint8)
    assert o.batch(u.ORACLE_ID[aead], 1, karr, 32, kidx, pt, ref, offs64, lens64, nonce_arr, nl,
                   ad_arr, ad_offs, ad_lens, ref_tags, 16) == 0
    if expect:
        for i in range(n):
            assert ref[offs[i]:offs[i] + lens[i]].tobytes() == expect[0][i]
            assert ref_tags[16 * i:16 * i + 16].tobytes() == expect[1][i]

    d_nonce, d_ad = _t(nonce_arr), _t(ad_arr)
    d_ki = None if ki is None else _t(np.asarray(ki, np.int32))
    obj = ba.AEADCtx(aead, keys[0], 16) if ki is None else \
        ba.Keyset(aead, b"".join(keys), len(keys), 16)
    if stride is not None:
        assert len(set(lens)) == 1 and len(set(ad_lens)) == 1
        assert offs == [i * stride for i in range(n)]

    def call(fn, src, tags):
        w_in, d_in = dev_arena(src, BASE[route])
        w_out, d_out = (w_in, d_in) if inplace else dev_arena(np.full(size, FILL, np.uint8),
                                                              BASE[route])
        d_tags = _t(tags)
        d_st = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
        assert_route(route, d_in, d_out, stride)
        if stride is not None:
            b = ba.make_batch(n, d_in, d_out, d_tags, d_nonce, nl, d_ad, record_stride=stride,
                              record_len=lens[0], ad_stride=int(ad_lens[0]),
                              ad_len=int(ad_lens[0]), status=d_st, key_index=d_ki)
            assert b.offsets is None and b.lengths is None
        else:
            b = ba.make_batch(n, d_in, d_out, d_tags, d_nonce, nl, d_ad,
                              offsets=_t(offs64.astype(np.int64)),
                              lengths=_t(lens64.astype(np.int64)),
                              ad_offsets=_t(ad_offs.astype(np.int64)),
                              ad_lengths=_t(ad_lens.astype(np.int64)), status=d_st,
                              key_index=d_ki)
            assert b.offsets is not None
        fn(b)
        torch.cuda.synchronize()
        out, margin_ok = arena_out(w_out, d_out)
        return out, margin_ok, d_tags.cpu().numpy(), d_st.cpu().numpy()

    def differing(a, b):
        """Records whose bytes differ, and whether the pattern between them differs."""
        d = a != b
        return [i for i in range(n) if d[offs[i]:offs[i] + lens[i]].any()], bool(d[~inside].any())

    what = (aead, route, lens[0] if stride else "ragged", int(ad_lens[0]))
    out, margin_ok, tags, st = call(obj.seal_batch_device, pt, np.zeros(16 * n, np.uint8))
    assert differing(out, ref) == ([], False) and margin_ok, (what, "seal: [records], between")
    bad_tags = [i for i in range(n) if not np.array_equal(tags[16 * i:16 * i + 16],
                                                          ref_tags[16 * i:16 * i + 16])]
    assert bad_tags == [] and list(st) == [1] * n, (what, "seal: tags")

    # Open with two records damaged: a tag byte, and the last ciphertext byte
    # (the partial tail) of a record that has one -- else a second tag.
    bad_tag = n // 3
    nonzero = [i for i in range(n) if lens[i] and i != bad_tag]
    bad_ct = nonzero[len(nonzero) // 2] if nonzero else 2 * n // 3
    tags_bad, ct_bad = ref_tags.copy(), ref.copy()
    tags_bad[16 * bad_tag + bad_tag % 16] ^= 0x20
    if nonzero:
        ct_bad[offs[bad_ct] + lens[bad_ct] - 1] ^= 0x04
    else:
        tags_bad[16 * bad_ct + 15] ^= 0x80
    want = pt.copy()
    for i in (bad_tag, bad_ct):
        want[offs[i]:offs[i] + lens[i]] = 0
    out, margin_ok, _, st = call(obj.open_batch_device, ct_bad, tags_bad)
    assert differing(out, want) == ([], False) and margin_ok, (what, "open: [records], between")
    assert list(st) == [int(i not in (bad_tag, bad_ct)) for i in range(n)], (what, "open: status")


def shuffled(lens, n, seed):
    """n lengths: all of `lens`, then repeats, in a seeded order."""
    out = [lens[i % len(lens)] for i in range(n)]
    random.Random(seed).shuffle(out)
    return out


def ragged_offsets(lens, odd=False):
    """Record offsets with at least 16 pattern bytes after every record:
    multiples of 16, or all odd."""
    offs, pos = [], 1 if odd else 0
    for x in lens:
        offs.append(pos)
        pos = (pos + x + 16 + 15) // 16 * 16 + (1 if odd else 0)
    return offs, pos + 16


def stride_of(route, rlen):
    if route == "lines":   # the next multiple of 128 above the length
        return (rlen // 128 + 1) * 128
    if route == "quads":   # a multiple of 16 but not of 128
        s = (rlen + 15) // 16 * 16 + 16
        return s if s % 128 else s + 16
    return rlen + 3 if (rlen + 1) % 16 == 0 else rlen + 1  # records at every byte alignment


def records(aead, key, lens, ad_lens, kinds, seed):
    """(pts, ads, nonces): record i of lens[i] bytes with ad_lens[i] AD bytes
    and content kinds[i]."""
    rng = np.random.default_rng(seed)
    nonces = u.rand_nonces(aead, len(lens), rng)
    pa = [u.content(kinds[i], aead, key, nonces[i], lens[i], ad_lens[i], rng)
          for i in range(len(lens))]
    return [p for p, _ in pa], [a for _, a in pa], nonces


def uniform(aead, route, rlen, ad_len, *, kind="random", inplace=False, seed=0):
    key, s = u.key_of(), stride_of(route, rlen)
    pts, ads, nonces = records(aead, key, [rlen] * N, [ad_len] * N, [kind] * N,
                               seed + 1000 * rlen + ad_len)
    check(aead, [key], pts, ads, nonces, [i * s for i in range(N)], N * s + 16, route, stride=s,
          inplace=inplace)


# ---------------------------------------------------------------------------
# a. uniform layouts

LAYOUTS = [("lines", False), ("lines", True), ("quads", False), ("any", False)]
LAYOUT_IDS = ["lines", "lines-inplace", "quads", "any"]


@pytest.mark.parametrize("aead", u.AEADS)
@pytest.mark.parametrize("route,inplace", LAYOUTS, ids=LAYOUT_IDS)
def test_uniform_every_length(aead, route, inplace):
    """Every length of LENS, the AD length rotating through AD_LENS."""
    for i, rlen in enumerate(u.LENS):
        uniform(aead, route, rlen, u.AD_LENS[i % len(u.AD_LENS)], inplace=inplace)


@pytest.mark.parametrize("aead", u.AEADS)
@pytest.mark.parametrize("route,inplace", LAYOUTS, ids=LAYOUT_IDS)
def test_uniform_every_ad_length(aead, route, inplace):
    """All ten AD lengths (0..5 blocks) at records of 0 and 1 bytes (no lane
    has a data block in iteration 0 under sh = 1), 64 and 200 bytes."""
    for rlen in (0, 1, 64, 200):
        for ad_len in u.AD_LENS:
            uniform(aead, route, rlen, ad_len, inplace=inplace, seed=7)


@pytest.mark.parametrize("aead", u.AEADS)
@pytest.mark.parametrize("route,inplace", LAYOUTS, ids=LAYOUT_IDS)
def test_uniform_maximal_limbs(aead, route, inplace):
    """Ciphertext and AD of all 0xff, and of all zero, bytes."""
    for kind in ("ones", "zeros"):
        uniform(aead, route, 4 * 64 + 49, 33, kind=kind, inplace=inplace)


# ---------------------------------------------------------------------------
# b. ragged batches (the aligned kernels: a record not on a 16-byte boundary
# takes their byte path)

def ragged(aead, lens, ad_lens, seed, *, odd=False, inplace=False, nkeys=1, ki=None):
    n = len(lens)
    keys = [u.key_of(k) for k in range(nkeys)]
    rng = np.random.default_rng(seed)
    nonces = u.rand_nonces(aead, n, rng)
    pts, ads = [], []
    for i in range(n):
        p, a = u.content(u.KINDS[i % 3], aead, keys[ki[i] if ki else 0], nonces[i], lens[i],
                         ad_lens[i], rng)
        pts.append(p), ads.append(a)
    offs, size = ragged_offsets(lens, odd)
    assert all(x % 16 == (1 if odd else 0) for x in offs)
    check(aead, keys, pts, ads, nonces, offs, size, "ragged", ki=ki, inplace=inplace)


@pytest.mark.parametrize("aead", u.AEADS)
@pytest.mark.parametrize("layout", ["aligned", "odd", "inplace"])
def test_ragged(aead, layout):
    """All of LENS + LONG with AD of 0..5 blocks per record: each wave takes
    the lane-tree AD branch with every nab mod 2 in it."""
    lens = shuffled(u.LENS + u.LONG, N_RAGGED, 21)
    assert set(lens) == set(u.LENS + u.LONG)
    ad_lens = [u.AD_LENS[(i + i // 32) % len(u.AD_LENS)] for i in range(N_RAGGED)]
    assert all(max(ad_lens[w:w + 32]) > 16 for w in range(0, N_RAGGED, 32))
    ragged(aead, lens, ad_lens, 22, odd=layout == "odd", inplace=layout == "inplace")


@pytest.mark.parametrize("aead", u.AEADS)
@pytest.mark.parametrize("ads", ["0-16", "none"])
def test_ragged_one_block_ad(aead, ads):
    """AD of at most one block in every record (0 mixed with 1..16 bytes, or
    none at all): whole waves take the one-block AD branch (wmax <= 1)."""
    lens = shuffled(u.LENS, N_RAGGED, 23)
    short = (0, 1, 0, 16, 13, 0, 8, 15)
    ad_lens = [short[(i + i // 8) % len(short)] if ads == "0-16" else 0 for i in range(N_RAGGED)]
    assert max(ad_lens) <= 16
    if ads == "0-16":
        assert all({0, 1, 16} <= set(ad_lens[w:w + 32]) for w in range(0, N_RAGGED, 32))
    ragged(aead, lens, ad_lens, 24)


# ---------------------------------------------------------------------------
# c. keyset

def test_ragged_keyset():
    """Three keys, every wave of 32 records holding all three."""
    lens = shuffled(u.LENS + u.LONG, N_RAGGED, 25)
    ki = [(i + i // 5) % 3 for i in range(N_RAGGED)]
    assert all(set(ki[w:w + 32]) == {0, 1, 2} for w in range(0, N_RAGGED, 32))
    ad_lens = [u.AD_LENS[(i + i // 32) % len(u.AD_LENS)] for i in range(N_RAGGED)]
    ragged(CHACHA, lens, ad_lens, 26, nkeys=3, ki=ki)


# ---------------------------------------------------------------------------
# d. TLS 1.3 records: one extra byte per record (the inner type), the XT kernels

TLS_IV = bytes(range(1, 13))


def check_tls(recs, types, offs, size, *, stride=None, expect=None):
    """Seal and open TLS 1.3 records against the record layer restated on the
    oracle's AEAD (as test_gcm_steady_loop.py::test_extra_byte_8_lanes).
    `stride`: a uniform batch of 128-byte lines.  `expect`: (cts, tags) of
    solved records, cts including the type's byte."""
    version, key, n = 0x0304, u.key_of(), len(recs)
    lens = [len(r) for r in recs]
    expected = tls_util.tls_seal_restated(version, CHACHA, key, TLS_IV, 0, recs, types)
    if expect:
        for i in range(n):
            assert expected[i][1] + expected[i][2] == expect[0][i] + expect[1][i]
    arena = np.full(size, FILL, np.uint8)
    want = arena.copy()
    for i in range(n):
        arena[offs[i]:offs[i] + lens[i]] = np.frombuffer(recs[i], np.uint8)
        want[offs[i]:offs[i] + lens[i]] = np.frombuffer(expected[i][1], np.uint8)
    sealer = ba.TlsAead(ba.evp_aead_seal, version, CHACHA, key, TLS_IV, 0)
    pl, sl = sealer.prefix_len, sealer.suffix_len
    assert sl == 17
    w_in, d_in = dev_arena(arena, 0)
    w_body, d_body = dev_arena(np.full(size, FILL, np.uint8), 0)
    d_pre = torch.zeros(n * pl, dtype=torch.uint8, device=DEV)
    d_suf = torch.zeros(n * sl, dtype=torch.uint8, device=DEV)
    d_st = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    if stride is None:
        where = dict(offsets=_t(np.array(offs, np.int64)), lengths=_t(np.array(lens, np.int64)))
    else:
        # (XT + COAL: whole_lines)
        assert stride % 128 == 0 and (d_in.data_ptr() | d_body.data_ptr()) % 128 == 0
        assert len(set(lens)) == 1 and offs == [i * stride for i in range(n)]
        where = dict(record_stride=stride, record_len=lens[0])
    sealer.seal_records_device(ba.make_tls_records(
        n, d_in, d_body, d_pre, d_suf, types=_t(np.array(types, np.uint8)), status=d_st, **where))
    torch.cuda.synchronize()
    body, margin_ok = arena_out(w_body, d_body)
    what = (lens[0] if stride else "ragged",)
    assert np.array_equal(body, want) and margin_ok, what
    assert d_pre.cpu().numpy().tobytes() == b"".join(e[0] for e in expected), what
    suf = d_suf.cpu().numpy().tobytes()
    assert [i for i in range(n) if suf[sl * i:sl * i + sl] != expected[i][2]] == [], what
    assert list(d_st.cpu().numpy()) == [1] * n

    bad = n // 3
    d_suf[bad * sl + 5] ^= 1
    opener = ba.TlsAead(ba.evp_aead_open, version, CHACHA, key, TLS_IV, 0)
    w_out, d_out = dev_arena(np.full(size, FILL, np.uint8), 0)
    d_types = torch.zeros(n, dtype=torch.uint8, device=DEV)
    opener.open_records_device(ba.make_tls_records(
        n, d_body, d_out, d_pre, d_suf, types=d_types, status=d_st, **where))
    torch.cuda.synchronize()
    arena[offs[bad]:offs[bad] + lens[bad]] = 0
    out, margin_ok = arena_out(w_out, d_out)
    assert np.array_equal(out, arena) and margin_ok, what
    assert list(d_st.cpu().numpy()) == [int(i != bad) for i in range(n)], what
    assert [t for i, t in enumerate(d_types.cpu().numpy()) if i != bad] == \
        [t for i, t in enumerate(types) if i != bad], what


def tls_records(lens, seed):
    rng = random.Random(seed)
    return [rng.randbytes(x) for x in lens], [rng.choice([21, 22, 23]) for _ in lens]


def test_tls13_ragged():
    """All of LENS, ragged (the XT kernel)."""
    lens = shuffled(u.LENS, N_RAGGED, 27)
    recs, types = tls_records(lens, 28)
    offs, size = ragged_offsets(lens)
    check_tls(recs, types, offs, size)


def test_tls13_lines():
    """Uniform batches of 128-byte lines (XT + COAL) at the lengths where the
    inner-type byte starts a new Poly1305 block, ChaCha block or iteration."""
    for rlen in [64 * k + r for k in range(4) for r in (0, 15, 16, 47, 62, 63)]:
        s = stride_of("lines", rlen)
        recs, types = tls_records([rlen] * N, rlen)
        check_tls(recs, types, [i * s for i in range(N)], N * s + 16, stride=s)


# ---------------------------------------------------------------------------
# e. iovec records

@pytest.mark.parametrize("aead", u.AEADS)
def test_iovec_cuts(aead):
    """Every length of LENS from 64 up, cut at points of {1, 16, 63, 64, 65,
    len - 1}; every fifth record in 20-byte chunks throughout (a 64-byte block
    over three or more chunks); AD in two chunks; a third in place."""
    key = u.key_of()
    lens = [x for x in u.LENS if x >= 64]
    lens = shuffled(lens, 2 * len(lens), 29)
    n = len(lens)
    ad_lens = [u.AD_LENS[i % len(u.AD_LENS)] for i in range(n)]
    pts, ads, nonces = records(aead, key, lens, ad_lens, [u.KINDS[i % 3] for i in range(n)], 30)
    rng = random.Random(31)
    chunks, starts, ad_chunks, ad_starts = [], [0], [], [0]
    pos, apos = 0, 0
    for i in range(n):
        x = lens[i]
        if i % 5 == 4:
            cuts = list(range(20, x, 20))
        else:
            points = [1, 16, 63, 64, 65, x - 1]
            cuts = sorted(c for c in {points[(i + j) % 6] for j in range(1 + i % 4)} if 0 < c < x)
        assert all(0 < c < x for c in cuts)
        prev = 0
        for c in cuts + [x]:
            pos += rng.randint(0, 7)
            chunks.append((pos, pts[i][prev:c], i % 3 == 0))
            pos += c - prev
            prev = c
        starts.append(len(chunks))
        cut = len(ads[i]) // 2
        for part in (ads[i][:cut], ads[i][cut:]):
            apos += rng.randint(0, 3)
            ad_chunks.append((apos, part))
            apos += len(part)
        ad_starts.append(len(ad_chunks))
    arena = IovArena(chunks, starts, ad_chunks, ad_starts, nonces)
    arena.d_dst.fill_(FILL)
    src_before = arena.d_src.cpu().numpy()
    ctx = ba.AEADCtx(aead, key, 16)
    cts, tags, st = arena.seal(ctx)
    assert st.tolist() == [1] * n
    for i in range(n):
        ok, ct, tag = o.seal(u.ORACLE_ID[aead], key, nonces[i], pts[i], ads[i])
        assert ok and cts[i] == ct and tags[16 * i:16 * i + 16].tobytes() == tag, (i, lens[i])
    # Outside the chunks written, both arenas are as they were.
    src_after, dst_after = arena.d_src.cpu().numpy(), arena.d_dst.cpu().numpy()
    in_src, in_dst = np.zeros(src_after.size, bool), np.zeros(dst_after.size, bool)
    for off, part, in_place in chunks:
        (in_src if in_place else in_dst)[off:off + len(part)] = True
    assert np.array_equal(src_after[~in_src], src_before[~in_src])
    assert (dst_after[~in_dst] == FILL).all()
    bad = set(range(0, n, 7))
    tg = tags.copy()
    for i in bad:
        tg[16 * i + i % 16] ^= 1
    back, st = arena.open(ctx, tg)
    for i in range(n):
        if i in bad:
            assert st[i] == 0 and back[i] == bytes(lens[i]), i
        else:
            assert st[i] == 1 and back[i] == pts[i], i


# ---------------------------------------------------------------------------
# f. solved accumulators: p - 1, 2^128, the all-zero and all-0xff tags, ...
# after the 4-block-unit Horner loop and the lane tree of every batch route

@pytest.mark.parametrize("aead", u.AEADS)
@pytest.mark.parametrize("batch", ["lines", "any", "ragged"])
def test_solved_accumulators(aead, batch):
    lens, ad_len, seed = u.SOLVED[batch]
    key = u.key_of()
    pts, ads, nonces, cts, tags, _ = u.solved_batch(aead, key, lens, ad_len, seed)
    if batch == "ragged":
        offs, size = ragged_offsets(lens)
        check(aead, [key], pts, ads, nonces, offs, size, "ragged", expect=(cts, tags))
    else:
        s = stride_of(batch, lens[0])
        check(aead, [key], pts, ads, nonces, [i * s for i in range(len(lens))], len(lens) * s + 16,
              batch, stride=s, expect=(cts, tags))


def test_solved_accumulators_tls13():
    recs, types, cts, tags, _ = u.tls_solved_batch(u.key_of(), TLS_IV)
    offs, size = ragged_offsets(u.TLS_SOLVED_LENS)
    check_tls(recs, types, offs, size, expect=(cts, tags))


# ---------------------------------------------------------------------------
# g. the one-record kernel, through the host API

def one_record(ctx, aead, key, nonce, pt, ad, expect=None):
    """ctx.seal equals the oracle's (and `expect`), ctx.open returns the
    plaintext, and a flipped last ciphertext byte (of an empty record: tag
    byte) is rejected."""
    ok, ct, tag = o.seal(u.ORACLE_ID[aead], key, nonce, pt, ad)
    assert ok and (expect is None or (ct, tag) == expect)
    what = (aead, len(ad), len(pt))
    assert ctx.seal(nonce, pt, ad) == ct + tag, what
    assert ctx.open(nonce, ct + tag, ad) == pt, what
    bad = bytearray(ct + tag)
    bad[len(ct) - 1 if ct else 0] ^= 0x01
    with pytest.raises(ba.AEADError) as e:
        ctx.open(nonce, bytes(bad), ad)
    assert e.value.lib == ba.ERR_LIB_CIPHER, what


def takes_one_record_kernel(ad_len, n):
    """chacha.hip one_record_batch, for a host record."""
    return n <= u.ONE_MAX_LEN and (ad_len + 15) // 16 + (n + 15) // 16 + 1 <= u.ONE_MAX_NBLK


@pytest.mark.parametrize("aead", u.AEADS)
def test_one_record_chunk_shapes(aead):
    """Every chunk size c = 1..8 of the 64- and 256-chunk trees with pad = 0
    and with the longest front padding, the switch at 512 / 513 blocks, and
    the hand-over to the batch kernel past 2,048 blocks or 16 KiB."""
    key, rng = u.key_of(), np.random.default_rng(41)
    ctx = ba.AEADCtx(aead, key, 16)
    cases = [u.one_lengths(nblk, odd) for nblk in u.ONE_NBLK for odd in (False, True)]
    assert all(takes_one_record_kernel(a, n) for a, n in cases)
    beyond = [u.one_lengths(2049, False), u.one_lengths(2049, True), (0, 16385)]
    assert not any(takes_one_record_kernel(a, n) for a, n in beyond)
    for ad_len, n in cases + beyond:
        nonce = u.rand_nonces(aead, 1, rng)[0]
        pt, ad = u.content("random", aead, key, nonce, n, ad_len, rng)
        one_record(ctx, aead, key, nonce, pt, ad)


@pytest.mark.parametrize("aead", u.AEADS)
def test_one_record_inline_ad(aead):
    """AD of 16 bytes goes by value (BatchDesc::inl), of 17 through memory."""
    key, rng = u.key_of(), np.random.default_rng(42)
    ctx = ba.AEADCtx(aead, key, 16)
    for ad_len in (0, 1, 15, 16, 17):
        for n in (0, 1, 64):
            nonce = u.rand_nonces(aead, 1, rng)[0]
            for kind in ("random", "ones"):
                pt, ad = u.content(kind, aead, key, nonce, n, ad_len, rng)
                one_record(ctx, aead, key, nonce, pt, ad)


@pytest.mark.parametrize("aead", u.AEADS)
@pytest.mark.parametrize("nblk", u.ONE_SOLVED_NBLK)
def test_one_record_solved(aead, nblk):
    key = u.key_of()
    ctx = ba.AEADCtx(aead, key, 16)
    assert takes_one_record_kernel(*u.one_lengths(nblk, False))
    for _, nonce, ad, pt, ct, tag in u.one_solved(aead, key, nblk, nblk):
        one_record(ctx, aead, key, nonce, pt, ad, expect=(ct, tag))


@pytest.mark.parametrize("aead", u.AEADS)
def test_one_record_maximal_limbs(aead):
    key, rng = u.key_of(), np.random.default_rng(43)
    ctx = ba.AEADCtx(aead, key, 16)
    for nblk in u.ONE_ONES_NBLK:
        for odd in (False, True):
            ad_len, n = u.one_lengths(nblk, odd)
            nonce = u.rand_nonces(aead, 1, rng)[0]
            pt, ad = u.content("ones", aead, key, nonce, n, ad_len, rng)
            one_record(ctx, aead, key, nonce, pt, ad)
