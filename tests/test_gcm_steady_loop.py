"""The whole-block steady loop of the AES-GCM bulk kernels (gcm.hip
process_records) against the CPU oracle, bit for bit.

A wave runs the steps in which every live record has a whole block in every
lane through a branch-free loop, D = 3 steps per trip (GCM_STEADY_DEPTH),
which stops D - 1 whole steps short and hands the rest to the general loop.
With B = 16 L bytes per step the lengths n B + r, n = 0..10, r in {0, 1, 15,
16, 17, B - 16, B - 1}, put 0, 1 and 2 trips, with every count of whole steps
left over, in front of every kind of tail (n = 0..7 do the same for two steps
per trip).  Uniform batches have 67 records and ragged ones 134 (they hold
all 77 lengths), so the last unit has dead records, and each lane count is
reached as launch_nr routes it.

Seal: ciphertext, tags and status equal the oracle's.  Open: of the sealed
batch with one record's tag flipped; that record gets status 0 and zeroed
output, the others their plaintext.  The space between and after the records
holds a pattern that must come back untouched.
"""
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import boringssl_amd as ba  # noqa: E402
import ctr_edge_util as u  # noqa: E402
import oracle_lib as o  # noqa: E402
import tls_util  # noqa: E402
from test_gpu_parity import DEV, _t  # noqa: E402

pytestmark = pytest.mark.gpu

N = 67
N_RAGGED = 134
FILL = 0x5a
KEYLEN = {"aes-128-gcm": 16, "aes-256-gcm": 32}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    ba.lib.ERR_clear_error()
    yield
    torch.cuda.synchronize()


def step_lens(lanes):
    """n B + r for n = 0..10 and every r of the module docstring (77 lengths)."""
    b = 16 * lanes
    return [n * b + r for n in range(11) for r in (0, 1, 15, 16, 17, b - 16, b - 1)]


def key_of(aead, k=0):
    return o.synth_key(1000 + k, KEYLEN[aead])


def ragged_offsets(lens, align=16, gap=16):
    """Record offsets with at least `gap` pattern bytes after every record."""
    offs, pos = [], 0
    for x in lens:
        offs.append(pos)
        pos = (pos + x + gap + align - 1) // align * align
    return offs, pos + 16


def check(aead, keys, lens, offs, size, *, ki=None, uniform=None, inplace=False, nonces=None,
          seed=1):
    """Seal and open one batch of records of lens[i] bytes at offs[i] in an
    arena of `size` bytes.  `uniform` = (stride, record_len): no per-record
    arrays.  `nonces`: byte strings of one length (default: random 12-byte)."""
    n = len(lens)
    rng = np.random.default_rng(seed)
    lens64, offs64 = np.asarray(lens, np.uint64), np.asarray(offs, np.uint64)
    if nonces is None:
        nl, nonce_arr = 12, rng.integers(0, 256, 12 * n, dtype=np.uint8)
    else:
        nl, nonce_arr = len(nonces[0]), np.frombuffer(b"".join(nonces), np.uint8).copy()
    ads = rng.integers(0, 256, 13 * n, dtype=np.uint8)
    inside = np.zeros(size, bool)
    for i in range(n):
        inside[offs[i]:offs[i] + lens[i]] = True
    pt = np.full(size, FILL, np.uint8)
    pt[inside] = rng.integers(0, 256, int(inside.sum()), dtype=np.uint8)

    karr = np.frombuffer(b"".join(keys), np.uint8).copy()
    kidx = None if ki is None else np.asarray(ki, np.uint32)
    ref = np.full(size, FILL, np.uint8)
    ref_tags = np.zeros(16 * n, np.uint8)
    ad_offs, ad_lens = np.arange(n, dtype=np.uint64) * np.uint64(13), np.full(n, 13, np.uint64)
    assert o.batch(o.AES_GCM, 1, karr, len(keys[0]), kidx, pt, ref, offs64, lens64, nonce_arr, nl,
                   ads, ad_offs, ad_lens, ref_tags, 16) == 0

    d_nonce, d_ad = _t(nonce_arr), _t(ads)
    d_ki = None if ki is None else _t(np.asarray(ki, np.int32))
    if ki is None:
        obj = ba.AEADCtx(aead, keys[0], 16)
    else:
        obj = ba.Keyset(aead, b"".join(keys), len(keys), 16)

    def call(fn, src, tags):
        d_in = _t(src)
        d_out = d_in if inplace else torch.full((size,), FILL, dtype=torch.uint8, device=DEV)
        d_tags = _t(tags)
        d_st = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
        if uniform:
            b = ba.make_batch(n, d_in, d_out, d_tags, d_nonce, nl, d_ad, record_stride=uniform[0],
                              record_len=uniform[1], ad_stride=13, ad_len=13, status=d_st,
                              key_index=d_ki)
        else:
            b = ba.make_batch(n, d_in, d_out, d_tags, d_nonce, nl, d_ad,
                              offsets=_t(offs64.astype(np.int64)),
                              lengths=_t(lens64.astype(np.int64)), ad_stride=13, ad_len=13,
                              status=d_st, key_index=d_ki)
        fn(b)
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), d_tags.cpu().numpy(), d_st.cpu().numpy()

    def differing(a, b):
        """Records whose bytes differ, and whether the pattern outside differs."""
        d = a != b
        return [i for i in range(n) if d[offs[i]:offs[i] + lens[i]].any()], bool(d[~inside].any())

    out, tags, st = call(obj.seal_batch_device, pt, np.zeros(16 * n, np.uint8))
    assert differing(out, ref) == ([], False), (lens, "seal: [records], outside")
    assert np.array_equal(tags, ref_tags) and list(st) == [1] * n

    bad = n // 3
    tags_bad = ref_tags.copy()
    tags_bad[16 * bad + bad % 16] ^= 0x20
    want = pt.copy()
    want[offs[bad]:offs[bad] + lens[bad]] = 0
    out, _, st = call(obj.open_batch_device, ref, tags_bad)
    assert differing(out, want) == ([], False), (lens, "open: [records], outside")
    assert list(st) == [int(i != bad) for i in range(n)]


def shuffled(lens, n, seed):
    """n lengths: all of `lens`, then repeats, in a seeded order."""
    out = [lens[i % len(lens)] for i in range(n)]
    random.Random(seed).shuffle(out)
    return out


# ---------------------------------------------------------------------------
# 8 lanes per record

def stride_8(rlen):
    """A multiple of 16 but not of 64, with pattern bytes after the record."""
    s = (rlen + 15) // 16 * 16 + 16
    return s if s % 64 else s + 16


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("aead", ["aes-128-gcm", "aes-256-gcm"])
def test_uniform_8_lanes(aead, inplace):
    """Uniform batches at a stride of 16 k bytes, 64 not dividing it."""
    for rlen in step_lens(8):
        s = stride_8(rlen)
        check(aead, [key_of(aead)], [rlen] * N, [i * s for i in range(N)], N * s + 16,
              uniform=(s, rlen), inplace=inplace, seed=rlen)


def test_ragged_8_lanes():
    """Fewer than 4,096 records of mixed lengths, those of five steps or more
    first: their waves mix trip counts (the minimum decides), the others
    mostly have none."""
    lens = shuffled(step_lens(8), N_RAGGED, 8)
    lens.sort(key=lambda x: x < 5 * 128)  # (stable: shuffled within each half)
    assert len({x // 128 for x in lens[:8]}) > 2 and min(lens[:64]) >= 5 * 128
    offs, size = ragged_offsets(lens)
    check("aes-128-gcm", [key_of("aes-128-gcm")], lens, offs, size)


def test_extra_byte_8_lanes():
    """TLS 1.3 records (one extra byte, the inner type): the XT kernel at 8
    lanes, against the record layer restated on the oracle's AEAD."""
    aead, version = "aes-128-gcm", 0x0304
    rng = random.Random(13)
    key, iv = key_of(aead), bytes(rng.getrandbits(8) for _ in range(12))
    n = N_RAGGED
    lens = shuffled(step_lens(8), n, 13)
    records = [bytes(rng.getrandbits(8) for _ in range(x)) for x in lens]
    types = [rng.choice([21, 22, 23]) for _ in range(n)]
    expect = tls_util.tls_seal_restated(version, aead, key, iv, 0, records, types)
    offs, size = ragged_offsets(lens)
    arena = np.full(size, FILL, np.uint8)
    want = arena.copy()
    for i in range(n):
        arena[offs[i]:offs[i] + lens[i]] = np.frombuffer(records[i], np.uint8)
        want[offs[i]:offs[i] + lens[i]] = np.frombuffer(expect[i][1], np.uint8)
    sealer = ba.TlsAead(ba.evp_aead_seal, version, aead, key, iv, 0)
    pl, sl = sealer.prefix_len, sealer.suffix_len
    d_body = torch.full((size,), FILL, dtype=torch.uint8, device=DEV)
    d_pre = torch.zeros(n * pl, dtype=torch.uint8, device=DEV)
    d_suf = torch.zeros(n * sl, dtype=torch.uint8, device=DEV)
    d_st = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    d_offs, d_lens = _t(np.array(offs, np.int64)), _t(np.array(lens, np.int64))
    sealer.seal_records_device(ba.make_tls_records(
        n, _t(arena), d_body, d_pre, d_suf, offsets=d_offs, lengths=d_lens,
        types=_t(np.array(types, np.uint8)), status=d_st))
    torch.cuda.synchronize()
    assert np.array_equal(d_body.cpu().numpy(), want)
    assert d_pre.cpu().numpy().tobytes() == b"".join(e[0] for e in expect)
    assert d_suf.cpu().numpy().tobytes() == b"".join(e[2] for e in expect)
    assert list(d_st.cpu().numpy()) == [1] * n

    bad = n // 3
    d_suf[bad * sl + 5] ^= 1
    opener = ba.TlsAead(ba.evp_aead_open, version, aead, key, iv, 0)
    d_out = torch.full((size,), FILL, dtype=torch.uint8, device=DEV)
    d_types = torch.zeros(n, dtype=torch.uint8, device=DEV)
    opener.open_records_device(ba.make_tls_records(
        n, d_body, d_out, d_pre, d_suf, offsets=d_offs, lengths=d_lens, types=d_types,
        status=d_st))
    torch.cuda.synchronize()
    arena[offs[bad]:offs[bad] + lens[bad]] = 0
    assert np.array_equal(d_out.cpu().numpy(), arena)
    assert list(d_st.cpu().numpy()) == [int(i != bad) for i in range(n)]
    assert [t for i, t in enumerate(d_types.cpu().numpy()) if i != bad] == \
        [t for i, t in enumerate(types) if i != bad]


# ---------------------------------------------------------------------------
# 4 lanes per record, and the length-ordered split

def test_uniform_4_lanes():
    """Uniform batches at a stride of 64 k bytes, records up to 4,096 bytes."""
    assert max(step_lens(4)) <= 4096
    aead = "aes-128-gcm"
    for rlen in step_lens(4):
        s = (rlen // 64 + 1) * 64
        check(aead, [key_of(aead)], [rlen] * N, [i * s for i in range(N)], N * s + 16,
              uniform=(s, rlen), seed=rlen)


def test_length_ordered_split():
    """4,099 ragged records: the short class at 4 lanes, the long one
    (4,096 + n B + r bytes) at 8, each in length order."""
    aead = "aes-128-gcm"
    lens = shuffled(step_lens(4) + step_lens(8), 4099 - 77, 4) + [4096 + x for x in step_lens(8)]
    random.Random(48).shuffle(lens)
    assert len(lens) >= 4096  # (wants_length_order)
    offs, size = ragged_offsets(lens)
    check(aead, [key_of(aead)], lens, offs, size)


# ---------------------------------------------------------------------------
# 16 lanes per record

def test_keyset_16_lanes():
    """Three keys, ragged: every pass of the tile has inactive groups."""
    aead = "aes-128-gcm"
    lens = shuffled(step_lens(16), N_RAGGED, 16)
    ki = [(i + i // 5) % 3 for i in range(N_RAGGED)]
    assert set(ki) == {0, 1, 2}
    offs, size = ragged_offsets(lens)
    check(aead, [key_of(aead, k) for k in range(3)], lens, offs, size, ki=ki)


def test_unaligned_uniform_16_lanes():
    """4,097-byte records at a 4,097-byte stride."""
    aead = "aes-128-gcm"
    check(aead, [key_of(aead)], [4097] * N, [i * 4097 for i in range(N)], N * 4097 + 16,
          uniform=(4097, 4097))


# ---------------------------------------------------------------------------
# the window-cache refresh inside the steady loop

@pytest.mark.parametrize("lanes,stride", [(8, 8336), (16, 8321)])
def test_window_refresh(lanes, stride):
    """8,320-byte records (520 blocks) under 16-byte nonces crafted so that,
    record by record, a block of a middle step receives the counter that
    wrapped to 0, or whose byte 2 or byte 3 carried: lanes of one wave enter
    new 256-counter windows in different steps."""
    aead, rlen = "aes-128-gcm", 8320
    assert (stride % 16 == 0 and stride % 64 != 0) if lanes == 8 else stride % 16 != 0
    key = key_of(aead)
    steps = rlen // (16 * lanes)
    nonces = []
    for i in range(N):
        cls = ("wrap", "carry2", "carry3")[i % 3]
        step = 2 + (i * 7) % (steps - 5)  # a middle step, odd and even
        w = step * lanes + (i * 5) % lanes
        assert lanes <= w < rlen // 16 - 2 * lanes
        nonces.append(u.gcm_record(key, rlen, (cls, w, w), f"steady/{lanes}/{i}")[0])
    check(aead, [key], [rlen] * N, [i * stride for i in range(N)], N * stride + 16,
          uniform=(stride, rlen), nonces=nonces)
